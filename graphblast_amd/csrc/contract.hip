// contract.hip -- graph contraction on the device: grb_relabel and grb_contract.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definitions are this project's own:
//   grb_relabel   map(v) = the number of distinct labels smaller than L(v): flags over 0 .. n - 1, the library's scan, a gather.
//   grb_contract  C = S^T A S with S(v, map(v)) = 1, the contributions to one C(a, b) folded under PLUS, MINIMUM, MAXIMUM or
//                 FIRST; sizes(a) = the vertices mapped to a.
// One sort-based path serves every operator and every coarse row, in a fixed number of plain launches:
//   1. ct_map_kernel     the range check of map, the dropped vertices, the histogram of the coarse ids (= sizes).
//   2. ct_keys_kernel    every stored A(i, j) gets the key (map(i) << cb | map(j)), cb = the bits of nc, and its CSR position
//                        as payload; an entry that does not survive (an end dropped; a loop when loops = 0) gets the key
//                        nc << cb, above every other.  kept and loops are counted here.  The host reads the record once.
//   3. device_sort_pairs_range over the 2 cb bits that matter.  The sort is stable and the payloads start ascending, so the
//                        contributions to one (a, b) -- a run -- stay in CSR position order = the order of (i, j).
//   4. ct_heads_kernel, the scan, ct_starts_kernel: run r begins at starts[r]; the scan's total is nvals(C), read by the host.
//   5. ct_ptr_kernel     C's row pointers by a search per coarse row; ct_fold_kernel: a lane per run.  FIRST copies the bits at
//                        the run's first position.  A run of up to kCtLaneRun contributions is folded by its lane in position
//                        order.  A longer one is cut into pieces of kCtPiece contributions -- a shape that depends on the run's
//                        length alone -- and queued: ct_piece_kernel folds a piece per wave (lane l takes l, l + 64, ..., then
//                        a butterfly), ct_final_kernel folds a run's piece results the same way.  One run of sixteen million
//                        contributions is 8192 pieces and one wave's fold of them, not a serial chain.
//   6. C's CSC is the transpose of that CSR (transpose_side, the path behind grb_transpose): never a second fold.
// PLUS on f32 adds in f64 and rounds once; MINIMUM / MAXIMUM compare the monotone map of the bits and map the winner back, so
// the winner's bits come out whatever the order; i32 PLUS wraps.  No floating-point atomic anywhere: the same inputs give the
// same bits whatever the grid.  Every index read from map or A is checked against its array before it is used.
#include "graph_common.hpp"

namespace grb {

constexpr int kCtLaneRun = 32;                           // a run of up to this many contributions: one lane folds it in order
constexpr int kCtPiece = 2048;                           // a longer run: pieces of this many, a wave each
enum { CT_PLUS_I32 = 0, CT_PLUS_F32, CT_MIN, CT_MAX, CT_FIRST };
// the call's record on the device (64-bit words, zero before the first kernel)
enum { kCtBad = 0, kCtDropped, kCtKept, kCtLoops, kCtLong /* long runs << 32 | their pieces */, kCtClusters, kCtLargest, kCtRecWords = 8 };

// ---- the fold ----------------------------------------------------------------------------------------------------------------
template <int M> struct CtAcc { typedef unsigned type; };
template <> struct CtAcc<CT_PLUS_F32> { typedef double type; };

template <int M>
__device__ __forceinline__ typename CtAcc<M>::type ct_identity() {
  if constexpr (M == CT_PLUS_F32) return -0.0;           // (-0 + x = x for every x, -0 included)
  else if constexpr (M == CT_MIN) return ~0u;            // (a real key at most: every run has a contribution)
  else return 0u;
}
template <int M>
__device__ __forceinline__ typename CtAcc<M>::type ct_load(unsigned bits, int f32) {
  if constexpr (M == CT_PLUS_F32) return (double)__uint_as_float(bits);
  else if constexpr (M == CT_MIN || M == CT_MAX) return value_order(bits, f32);
  else return bits;
}
template <int M>
__device__ __forceinline__ typename CtAcc<M>::type ct_combine(typename CtAcc<M>::type x, typename CtAcc<M>::type y) {
  if constexpr (M == CT_MIN) return x < y ? x : y;
  else if constexpr (M == CT_MAX) return x > y ? x : y;
  else return x + y;
}
template <int M>
__device__ __forceinline__ unsigned ct_store(typename CtAcc<M>::type x, int f32) {
  if constexpr (M == CT_PLUS_F32) return __float_as_uint((float)x);
  else if constexpr (M == CT_MIN || M == CT_MAX) return value_unorder(x, f32);
  else return x;
}
template <int M>
__device__ __forceinline__ unsigned long long ct_bits(typename CtAcc<M>::type x) {
  if constexpr (M == CT_PLUS_F32) return (unsigned long long)__double_as_longlong(x);
  else return (unsigned long long)x;
}
template <int M>
__device__ __forceinline__ typename CtAcc<M>::type ct_from(unsigned long long u) {
  if constexpr (M == CT_PLUS_F32) return __longlong_as_double((long long)u);
  else return (unsigned)u;
}
template <int M>
__device__ __forceinline__ typename CtAcc<M>::type ct_butterfly(typename CtAcc<M>::type x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = ct_combine<M>(x, __shfl_xor(x, o, kWave));
  return x;
}

// ---- vectors -------------------------------------------------------------------------------------------------------------------
// a sparse vector with every value stored: out (filled with a value out of every range before) gets them at their indices
__global__ __launch_bounds__(kBlock) void ct_scatter_kernel(const Index* __restrict__ ind, const int* __restrict__ val, Index nvals, Index n,
                                                            int* __restrict__ out) {
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < nvals; k += (long long)gridDim.x * kBlock)
    if ((unsigned)ind[k] < (unsigned)n) out[ind[k]] = val[k];
}

// L(v) of grb_relabel; false: labels(v) is out of range
__device__ __forceinline__ bool rl_label(int l, long long v, long long n, int kind, Index* out) {
  if (kind == GRB_RELABEL_LABELS) {
    *out = (Index)l;
    return (unsigned)l < (unsigned)n;
  }
  *out = l < 0 || (long long)l > v ? (Index)v : (Index)l;
  return l >= -1 && (long long)l < n;
}
// flags[L(v)] = 1 (flags: n + 1 words, zero before; plain stores of the same value); rec[kCtBad] |= 1 for a label out of range
__global__ __launch_bounds__(kBlock) void rl_mark_kernel(const int* __restrict__ labels, long long n, int kind, unsigned* __restrict__ flags,
                                                         unsigned long long* __restrict__ rec) {
  bool bad = false;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    Index L;
    if (rl_label(labels[v], v, n, kind, &L)) flags[L] = 1u;
    else bad = true;
  }
  if (bad) atomicOr(&rec[kCtBad], 1ull);
}
// out(v) = the scanned flags at L(v): the distinct labels below it
__global__ __launch_bounds__(kBlock) void rl_gather_kernel(const int* __restrict__ labels, long long n, int kind, const unsigned* __restrict__ ranks,
                                                           int* __restrict__ out) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    Index L;
    out[v] = rl_label(labels[v], v, n, kind, &L) ? (int)ranks[L] : -1;       // (the host has seen the flag by then: never -1)
  }
}

// ---- grb_contract ----------------------------------------------------------------------------------------------------------------
// the range check of map (-1 .. nc - 1), the dropped vertices, sizes[a] = |{v : map(v) = a}| (zero before).  A wave whose
// vertices share one coarse id -- the giant cluster -- adds once.
__global__ __launch_bounds__(kBlock) void ct_map_kernel(const int* __restrict__ map, long long n, Index nc, unsigned* __restrict__ sizes,
                                                        unsigned long long* __restrict__ rec) {
  const int lane = lane_id();
  bool bad = false;
  unsigned dropped = 0;
  for (long long base = (long long)blockIdx.x * kBlock; base < n; base += (long long)gridDim.x * kBlock) {
    const long long v = base + threadIdx.x;
    const int m = v < n ? map[v] : -1;
    const bool valid = v < n && (unsigned)m < (unsigned)nc;
    if (v < n && !valid) {
      if (m == -1) ++dropped; else bad = true;
    }
    const unsigned long long todo = __ballot(valid);
    if (todo == 0ull) continue;
    const int leader = __ffsll((long long)todo) - 1;
    const int lm = __shfl(m, leader, kWave);
    const unsigned long long peers = __ballot(valid && m == lm);
    if (lane == leader) atomicAdd(&sizes[lm], (unsigned)__popcll(peers));
    else if (valid && m != lm) atomicAdd(&sizes[m], 1u);
  }
  dropped = wave_sum_u32(dropped);
  if (lane == 0 && dropped) atomicAdd(&rec[kCtDropped], (unsigned long long)dropped);
  if (bad) atomicOr(&rec[kCtBad], 1ull);
}

// key and payload of every stored entry; the counts of the kept entries and of the loops among them
__global__ __launch_bounds__(kBlock) void ct_keys_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, const int* __restrict__ map,
                                                         Index n, long long nnz, Index nc, int cb, int loops,
                                                         unsigned long long* __restrict__ keys, unsigned* __restrict__ pay,
                                                         unsigned long long* __restrict__ rec) {
  const unsigned long long gone = (unsigned long long)(unsigned)nc << cb;
  unsigned kept = 0, looped = 0;
  for (long long base = (long long)blockIdx.x * kBlock; base < nnz; base += (long long)gridDim.x * kBlock) {
    const long long e = base + threadIdx.x;
    if (e >= nnz) continue;
    Index lo = 0, hi = n;                                // the row: the last r with ptr[r] <= e
    while (hi - lo > 1) {
      const Index mid = lo + ((hi - lo) >> 1);
      if ((long long)ptr[mid] <= e) lo = mid; else hi = mid;
    }
    const Index j = ind[e];
    const int a = map[lo];
    const int b = (unsigned)j < (unsigned)n ? map[j] : -1;
    const bool keep = (unsigned)a < (unsigned)nc && (unsigned)b < (unsigned)nc;
    const bool loop = keep && a == b;
    kept += keep ? 1u : 0u;
    looped += loop ? 1u : 0u;
    keys[e] = keep && (loops || !loop) ? ((unsigned long long)(unsigned)a << cb) | (unsigned)b : gone;
    pay[e] = (unsigned)e;
  }
  kept = wave_sum_u32(kept);
  looped = wave_sum_u32(looped);
  if (lane_id() == 0) {
    if (kept) atomicAdd(&rec[kCtKept], (unsigned long long)kept);
    if (looped) atomicAdd(&rec[kCtLoops], (unsigned long long)looped);
  }
}

// flags[p] = 1 where a run begins among the first S sorted keys; flags[S] = 0: their exclusive scan numbers the runs
__global__ __launch_bounds__(kBlock) void ct_heads_kernel(const unsigned long long* __restrict__ keys, long long S, unsigned* __restrict__ flags) {
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p <= S; p += (long long)gridDim.x * kBlock)
    flags[p] = p < S && (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}
// starts[r] = the first position of run r; starts[E] = S
__global__ __launch_bounds__(kBlock) void ct_starts_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ runs, long long S,
                                                           unsigned* __restrict__ starts) {
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p <= S; p += (long long)gridDim.x * kBlock)
    if (p == S || p == 0 || keys[p] != keys[p - 1]) starts[runs[p]] = (unsigned)p;
}
// C's row pointers: optr[a] = the number of the first run of a coarse row >= a (a search per row, no histogram)
__global__ __launch_bounds__(kBlock) void ct_ptr_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ runs, long long S,
                                                        Index nc, int cb, Index* __restrict__ optr) {
  for (long long a = (long long)blockIdx.x * kBlock + threadIdx.x; a <= nc; a += (long long)gridDim.x * kBlock) {
    long long lo = 0, hi = S;
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if ((long long)(keys[mid] >> cb) < a) lo = mid + 1; else hi = mid;
    }
    optr[a] = (Index)runs[lo];                           // (runs[S] = E)
  }
}

// a lane per run: the column, and the value of a run of up to kCtLaneRun contributions; a longer one is queued with its pieces
template <int M>
__global__ __launch_bounds__(kBlock) void ct_fold_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ pay,
                                                         const unsigned* __restrict__ val, const unsigned* __restrict__ starts, long long E, int cb,
                                                         int f32, Index* __restrict__ oind, unsigned* __restrict__ oval,
                                                         unsigned* __restrict__ long_run, unsigned* __restrict__ long_base, unsigned cap,
                                                         unsigned long long* __restrict__ rec) {
  const unsigned long long colmask = (1ull << cb) - 1ull;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < E; r += (long long)gridDim.x * kBlock) {
    const unsigned p0 = starts[r], p1 = starts[r + 1];
    oind[r] = (Index)(keys[p0] & colmask);
    if (M == CT_FIRST) {
      oval[r] = val[pay[p0]];
      continue;
    }
    const unsigned len = p1 - p0;
    if (len <= (unsigned)kCtLaneRun) {
      typename CtAcc<M>::type acc = ct_load<M>(val[pay[p0]], f32);
      for (unsigned p = p0 + 1; p < p1; ++p) acc = ct_combine<M>(acc, ct_load<M>(val[pay[p]], f32));
      oval[r] = ct_store<M>(acc, f32);
    } else {
      const unsigned pieces = (len + kCtPiece - 1) / kCtPiece;
      const unsigned long long t = atomicAdd(&rec[kCtLong], (1ull << 32) | (unsigned long long)pieces);
      const unsigned slot = (unsigned)(t >> 32), base = (unsigned)t;
      if (slot < cap) {                                  // (always: a long run has more than kCtLaneRun contributions)
        long_run[slot] = (unsigned)r;
        long_base[slot] = base;                          // ascending in slot: one atomic hands out both
      }
    }
  }
}
// a wave per piece of a long run: lane l folds l, l + 64, ... in order, then the butterfly
template <int M>
__global__ __launch_bounds__(kBlock) void ct_piece_kernel(const unsigned* __restrict__ pay, const unsigned* __restrict__ val,
                                                          const unsigned* __restrict__ starts, int f32, const unsigned* __restrict__ long_run,
                                                          const unsigned* __restrict__ long_base, unsigned cap,
                                                          const unsigned long long* __restrict__ rec, unsigned long long* __restrict__ partial) {
  const int lane = lane_id();
  const unsigned long long t = rec[kCtLong];
  unsigned nlong = (unsigned)(t >> 32), npieces = (unsigned)t;
  if (nlong > cap) nlong = cap;                          // (never)
  if (npieces > cap) npieces = cap;
  const unsigned gwaves = gridDim.x * kWavesPerBlock;
  for (unsigned q = blockIdx.x * kWavesPerBlock + wave_id(); q < npieces; q += gwaves) {
    unsigned lo = 0, hi = nlong;                         // the run: the last slot with long_base[slot] <= q
    while (hi - lo > 1u) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      if (long_base[mid] <= q) lo = mid; else hi = mid;
    }
    const unsigned r = long_run[lo], k = q - long_base[lo];
    const unsigned long long b = (unsigned long long)starts[r] + (unsigned long long)k * kCtPiece, end = starts[r + 1];
    const unsigned long long e = b + kCtPiece < end ? b + kCtPiece : end;
    typename CtAcc<M>::type acc = ct_identity<M>();
    for (unsigned long long p = b + lane; p < e; p += kWave) acc = ct_combine<M>(acc, ct_load<M>(val[pay[p]], f32));
    acc = ct_butterfly<M>(acc);
    if (lane == 0) partial[q] = ct_bits<M>(acc);
  }
}
// a wave per long run: its pieces' results folded the same way
template <int M>
__global__ __launch_bounds__(kBlock) void ct_final_kernel(const unsigned* __restrict__ starts, int f32, const unsigned* __restrict__ long_run,
                                                          const unsigned* __restrict__ long_base, unsigned cap,
                                                          const unsigned long long* __restrict__ rec, const unsigned long long* __restrict__ partial,
                                                          unsigned* __restrict__ oval) {
  const int lane = lane_id();
  const unsigned long long t = rec[kCtLong];
  unsigned nlong = (unsigned)(t >> 32);
  if (nlong > cap) nlong = cap;                          // (never)
  const unsigned gwaves = gridDim.x * kWavesPerBlock;
  for (unsigned slot = blockIdx.x * kWavesPerBlock + wave_id(); slot < nlong; slot += gwaves) {
    const unsigned r = long_run[slot], base = long_base[slot];
    const unsigned len = starts[r + 1] - starts[r];
    unsigned pieces = (len + kCtPiece - 1) / kCtPiece;
    if ((unsigned long long)base + pieces > cap) pieces = base < cap ? cap - base : 0u;   // (never)
    typename CtAcc<M>::type acc = ct_identity<M>();
    for (unsigned q = lane; q < pieces; q += kWave) acc = ct_combine<M>(acc, ct_from<M>(partial[base + q]));
    acc = ct_butterfly<M>(acc);
    if (lane == 0) oval[r] = ct_store<M>(acc, f32);
  }
}

// the non-empty clusters and the largest one (sixteen ids a thread: two same-address atomics a wave)
__global__ __launch_bounds__(kBlock) void ct_sizes_kernel(const unsigned* __restrict__ sizes, long long nc, unsigned long long* __restrict__ rec) {
  unsigned used = 0, largest = 0;
  for (long long a = (long long)blockIdx.x * kBlock + threadIdx.x; a < nc; a += (long long)gridDim.x * kBlock) {
    const unsigned s = sizes[a];
    used += s ? 1u : 0u;
    largest = s > largest ? s : largest;
  }
  used = wave_sum_u32(used);
  largest = wave_max_u32(largest);
  if (lane_id() == 0) {
    if (used) atomicAdd(&rec[kCtClusters], (unsigned long long)used);
    if (largest) atomicMax(&rec[kCtLargest], (unsigned long long)largest);
  }
}

namespace {

inline int ct_sort_launches(int bits) { return 5 * ((bits + 7) / 8); }   // a histogram, the scan's three, a scatter per digit

// the stored values of an i32 vector with every value stored, as n words on the device: its dense storage, or `tmp` filled
// from its sparse storage (a value out of every range where an index is missing)
grb_info ct_dense_values(grb_vector u, Index n, int* tmp, hipStream_t s, const int** out) {
  if (u->vec_type == GRB_DENSE) {
    *out = (const int*)u->d_val;
    return GRB_SUCCESS;
  }
  GRB_HIP_TRY(hipMemsetAsync(tmp, 0x80, 4 * (size_t)n, s));
  hipLaunchKernelGGL(ct_scatter_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, u->s_ind, (const int*)u->s_val, n, n, tmp);
  GRB_HIP_TRY(hipGetLastError());
  *out = tmp;
  return GRB_SUCCESS;
}
inline Index ct_stored(const grb_vector_s* u) {
  return u->vec_type == GRB_DENSE ? u->nsize : u->vec_type == GRB_SPARSE ? u->s_nvals : 0;
}
grb_info relabel_run(grb_vector map, grb_vector labels, int kind, int32_t* count) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = labels->nsize;
  if (n == 0) {
    map->vec_type = GRB_DENSE;
    map->d_nnz = 0;
    if (count) *count = 0;
    return GRB_SUCCESS;
  }
  // ---- one allocation: the record, the flags, the result, the labels of a sparse vector, the scan's totals
  const size_t fw = pad_bytes(4 * ((size_t)n + 1)), scan_bytes = pad_bytes(device_scan_u32_scratch((long long)n + 1));
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 256 + 3 * fw + scan_bytes));
  unsigned long long* d_rec = (unsigned long long*)work.p;
  unsigned* d_flags = (unsigned*)((char*)work.p + 256);
  int* d_out = (int*)((char*)d_flags + fw);
  int* d_tmp = (int*)((char*)d_out + fw);
  unsigned* d_totals = (unsigned*)((char*)d_tmp + fw);
  GRB_TRY(dense_out_prepare(map, n));
  GRB_HIP_TRY(hipMemsetAsync(work.p, 0, 256 + fw, s));
  const int* d_lab = nullptr;
  GRB_TRY(ct_dense_values(labels, n, d_tmp, s, &d_lab));
  hipLaunchKernelGGL(rl_mark_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_lab, (long long)n, kind, d_flags, d_rec);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_flags, (long long)n + 1, d_totals));
  hipLaunchKernelGGL(rl_gather_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_lab, (long long)n, kind, (const unsigned*)d_flags, d_out);
  GRB_HIP_TRY(hipGetLastError());
  unsigned long long bad = 0;
  unsigned nc = 0;
  GRB_HIP_TRY(hipMemcpyAsync(&bad, d_rec + kCtBad, 8, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipMemcpyAsync(&nc, d_flags + n, 4, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // the call's one read
  if (bad) return GRB_INVALID_INDEX;
  GRB_TRY(dense_out_commit(map, d_out, n, s));
  if (count) *count = (int32_t)nc;
  return GRB_SUCCESS;
}

template <int M>
void ct_fold_launch(hipStream_t s, const unsigned long long* keys, const unsigned* pay, const unsigned* val, const unsigned* starts, long long E,
                    int cb, int f32, Index* oind, unsigned* oval, unsigned* long_run, unsigned* long_base, unsigned cap,
                    unsigned long long* rec, unsigned long long* partial, long long S) {
  hipLaunchKernelGGL(ct_fold_kernel<M>, dim3(stream_grid(E)), dim3(kBlock), 0, s, keys, pay, val, starts, E, cb, f32, oind, oval, long_run,
                     long_base, cap, rec);
  if (M == CT_FIRST || S <= kCtLaneRun) return;          // no run can be long
  const int grid = stream_grid(S / kCtPiece + S / (4 * kCtLaneRun) + 1, kWavesPerBlock);
  hipLaunchKernelGGL(ct_piece_kernel<M>, dim3(grid), dim3(kBlock), 0, s, pay, val, starts, f32, (const unsigned*)long_run,
                     (const unsigned*)long_base, cap, (const unsigned long long*)rec, partial);
  hipLaunchKernelGGL(ct_final_kernel<M>, dim3(grid), dim3(kBlock), 0, s, starts, f32, (const unsigned*)long_run, (const unsigned*)long_base, cap,
                     (const unsigned long long*)rec, (const unsigned long long*)partial, oval);
}

grb_info contract_run(grb_matrix C, grb_vector sizes, grb_matrix A, grb_vector map, int op, int loops, grb_contract_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = A->nrows, nc = C->nrows;
  const long long Z = n > 0 ? (long long)A->nvals : 0;
  const int f32 = A->dtype == GRB_F32 ? 1 : 0;
  const bool both = C->format != 1;
  grb_contract_result r = {};
  EventPair ev;
  GRB_TRY(ev.create());
  int cb = 1;                                            // nc < 2^cb: a coarse id and the key of a dropped entry fit
  while (cb < 31 && ((long long)1 << cb) <= (long long)nc) ++cb;
  // ---- one allocation: the record, keys, the pieces' results, payloads, flags, starts, the long runs, map, sizes, the scan
  const unsigned cap = (unsigned)(Z / kCtLaneRun + 2);   // long runs and pieces, at most (a long run of len has <= len / 32 pieces)
  const size_t kb = pad_bytes(8 * (size_t)(Z + 1)), pb = pad_bytes(8 * (size_t)cap), wb = pad_bytes(4 * (size_t)(Z + 2)), lb = pad_bytes(4 * (size_t)cap);
  const size_t nb = pad_bytes(4 * ((size_t)n + 1)), cbytes = pad_bytes(4 * ((size_t)nc + 1));
  const size_t scan_bytes = pad_bytes(device_scan_u32_scratch(Z + 2));
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 256 + kb + pb + 3 * wb + 2 * lb + nb + cbytes + scan_bytes));
  char* q = (char*)work.p;
  unsigned long long* d_rec = (unsigned long long*)q; q += 256;
  unsigned long long* d_keys = (unsigned long long*)q; q += kb;
  unsigned long long* d_partial = (unsigned long long*)q; q += pb;
  unsigned* d_pay = (unsigned*)q; q += wb;
  unsigned* d_flags = (unsigned*)q; q += wb;
  unsigned* d_starts = (unsigned*)q; q += wb;
  unsigned* d_long_run = (unsigned*)q; q += lb;
  unsigned* d_long_base = (unsigned*)q; q += lb;
  int* d_tmp = (int*)q; q += nb;
  unsigned* d_sizes = (unsigned*)q; q += cbytes;
  unsigned* d_totals = (unsigned*)q;
  if (sizes) GRB_TRY(dense_out_prepare(sizes, nc));
  Side sr, sc;
  GRB_TRY(ewm_alloc(&sr.ptr, 4 * ((size_t)nc + 1)));
  sr.h_ptr.assign((size_t)nc + 1, 0);
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 256, s));
  GRB_HIP_TRY(hipMemsetAsync(d_sizes, 0, cbytes, s));
  unsigned long long h[kCtRecWords] = {};
  long long S = 0, E = 0;
  int launches = 0;
  if (n > 0) {
    const int* d_map = nullptr;
    GRB_TRY(ct_dense_values(map, n, d_tmp, s, &d_map));
    launches += map->vec_type == GRB_DENSE ? 0 : 1;
    hipLaunchKernelGGL(ct_map_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_map, (long long)n, nc, d_sizes, d_rec);
    ++launches;
    if (Z > 0 && nc > 0) {
      hipLaunchKernelGGL(ct_keys_kernel, dim3(stream_grid(Z)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, d_map, n, Z, nc, cb, loops, d_keys,
                         d_pay, d_rec);
      ++launches;
    }
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(h, d_rec, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the first of the call's two reads: the check and the counts
    if (h[kCtBad]) return GRB_INVALID_INDEX;
    S = (long long)h[kCtKept] - (loops ? 0ll : (long long)h[kCtLoops]);
  }
  if (S > 0) {
    GRB_TRY(device_sort_pairs_range(d_keys, d_pay, Z, 0, 2 * cb));
    launches += ct_sort_launches(2 * cb);
    hipLaunchKernelGGL(ct_heads_kernel, dim3(stream_grid(S + 1)), dim3(kBlock), 0, s, (const unsigned long long*)d_keys, S, d_flags);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_exclusive_scan_u32_async(d_flags, S + 1, d_totals));
    hipLaunchKernelGGL(ct_starts_kernel, dim3(stream_grid(S + 1)), dim3(kBlock), 0, s, (const unsigned long long*)d_keys,
                       (const unsigned*)d_flags, S, d_starts);
    hipLaunchKernelGGL(ct_ptr_kernel, dim3(stream_grid((long long)nc + 1)), dim3(kBlock), 0, s, (const unsigned long long*)d_keys,
                       (const unsigned*)d_flags, S, nc, cb, (Index*)sr.ptr.p);
    GRB_HIP_TRY(hipGetLastError());
    launches += 6;
    unsigned runs = 0;
    GRB_HIP_TRY(hipMemcpyAsync(&runs, d_flags + S, 4, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)nc + 1), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the second: nvals(C)
    E = (long long)runs;
  } else {
    GRB_HIP_TRY(hipMemsetAsync(sr.ptr.p, 0, 4 * ((size_t)nc + 1), s));
  }
  GRB_TRY(ewm_alloc(&sr.ind, 4 * (size_t)(E > 0 ? E : 1)));
  GRB_TRY(ewm_alloc(&sr.val, 4 * (size_t)(E > 0 ? E : 1)));
  sr.nnz = (Index)E;
  if (E > 0) {
    const unsigned* val = (const unsigned*)A->csr.val;
    Index* oind = (Index*)sr.ind.p;
    unsigned* oval = (unsigned*)sr.val.p;
    const int mode = op == GRB_OP_FIRST ? CT_FIRST : op == GRB_OP_MINIMUM ? CT_MIN : op == GRB_OP_MAXIMUM ? CT_MAX : f32 ? CT_PLUS_F32 : CT_PLUS_I32;
#define GRB_CT_FOLD(MODE)                                                                                                          \
  case MODE:                                                                                                                       \
    ct_fold_launch<MODE>(s, d_keys, d_pay, val, d_starts, E, cb, f32, oind, oval, d_long_run, d_long_base, cap, d_rec, d_partial, S); \
    break;
    switch (mode) {
      GRB_CT_FOLD(CT_PLUS_I32) GRB_CT_FOLD(CT_PLUS_F32) GRB_CT_FOLD(CT_MIN) GRB_CT_FOLD(CT_MAX) GRB_CT_FOLD(CT_FIRST)
    }
#undef GRB_CT_FOLD
    GRB_HIP_TRY(hipGetLastError());
    launches += mode == CT_FIRST || S <= kCtLaneRun ? 1 : 3;
  }
  if (nc > 0) {
    hipLaunchKernelGGL(ct_sizes_kernel, dim3(stream_grid(nc, kBlock * 16)), dim3(kBlock), 0, s, (const unsigned*)d_sizes, (long long)nc, d_rec);
    GRB_HIP_TRY(hipGetLastError());
    ++launches;
  }
  GRB_HIP_TRY(hipMemcpyAsync(h, d_rec, sizeof(h), hipMemcpyDeviceToHost, s));
  // ---- the CSC: the transpose of the CSR just made (the path behind grb_transpose)
  if (both) {
    if (E > 0) {
      CsrArrays X;
      X.ptr = (Index*)sr.ptr.p;
      X.ind = (Index*)sr.ind.p;
      X.val = sr.val.p;
      X.n = nc;
      X.nvals = (Index)E;
      GRB_TRY(transpose_side(X, nc, nc, &sc));
      launches += 3 + ct_sort_launches(cb);
    } else {
      GRB_TRY(ewm_alloc(&sc.ptr, 4 * ((size_t)nc + 1)));
      GRB_TRY(ewm_alloc(&sc.ind, 4));
      GRB_TRY(ewm_alloc(&sc.val, 4));
      GRB_HIP_TRY(hipMemsetAsync(sc.ptr.p, 0, 4 * ((size_t)nc + 1), s));
      sc.h_ptr.assign((size_t)nc + 1, 0);
      sc.nnz = 0;
    }
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  r.kept = (int64_t)h[kCtKept];
  r.loops = (int64_t)h[kCtLoops];
  r.entries = (int64_t)E;
  r.clusters = (int32_t)h[kCtClusters];
  r.dropped = (int32_t)h[kCtDropped];
  r.largest = (int32_t)h[kCtLargest];
  r.launches = launches;
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches C) and one copy.  A, which
  // may be C, has been read for the last time
  GRB_TRY(attach(C, &sr, both ? &sc : nullptr));
  if (sizes) GRB_TRY(dense_out_commit(sizes, d_sizes, nc, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contracts are the comments in include/grb_hip.h
grb_info grb_relabel(grb_vector map, grb_vector labels, int kind, int32_t* count, grb_descriptor desc) { GRB_API_ENTER();
  (void)desc;
  if (!map || !labels) return GRB_UNINITIALIZED_OBJECT;
  if (map->nsize != labels->nsize) return GRB_DIMENSION_MISMATCH;
  if (map->dtype != GRB_I32 || labels->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  if (kind != GRB_RELABEL_LABELS && kind != GRB_RELABEL_MATE) return GRB_INVALID_VALUE;
  if (ct_stored(labels) != labels->nsize) return GRB_INVALID_VALUE;
  return relabel_run(map, labels, kind, count);
}

grb_info grb_contract(grb_matrix C, grb_vector sizes, grb_matrix A, grb_vector map, grb_binary_op op, int loops, grb_descriptor desc,
                      grb_contract_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!C || !A || !A->built || !map) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows, nc = C->nrows;
  if (A->nrows != A->ncols || C->nrows != C->ncols || map->nsize != n || (sizes && sizes->nsize != nc)) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || map->dtype != GRB_I32 || (sizes && sizes->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (C->dtype != A->dtype) return GRB_DOMAIN_MISMATCH;
  if (op != GRB_OP_PLUS && op != GRB_OP_MINIMUM && op != GRB_OP_MAXIMUM && op != GRB_OP_FIRST) return GRB_NOT_IMPLEMENTED;
  if ((loops != 0 && loops != 1) || ct_stored(map) != n) return GRB_INVALID_VALUE;
  if (n > 0 && A->nvals > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return contract_run(C, sizes, A, map, (int)op, loops, result);
}
