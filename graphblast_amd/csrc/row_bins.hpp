// row_bins.hpp -- the pipeline the matrix-producing ops share (ewise_matrix, extract, assign_matrix; spgemm uses the total
// and the helpers): the rows of the result are cut into three bins by a length the op defines, a symbolic pass counts every
// row, the counts are summed in 64 bits and scanned into row pointers, and a numeric pass over the same bins writes.
//   short  len <= kShortMax   a 16-lane group per row
//   wave   len <= kSeg        a wave per row
//   hub    the rest           the row cut into segments of kSeg, a wave each (seg_row / seg_k; seg_cnt: a segment's count,
//                             then, scanned, its offset)
// A row of length <= 0 is in no bin.  The tuning constants (the short bin's width, the segment length, the thresholds) and
// the merge / row kernels stay in their files: each op is retuned alone.
#pragma once
#include "common.hpp"

namespace grb {

// ---- device ----------------------------------------------------------------------------------------------------------------
// the lanes of a wave see each other's LDS writes
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// -1 none (empty), 0 short, 1 wave, 2 hub
template <int kShortMax, int kSeg>
__device__ inline int row_bin_of(long long len) { return len <= 0 ? -1 : len <= kShortMax ? 0 : len <= kSeg ? 1 : 2; }

// rows -> bin lists.  len_of(i) is row i's length (a small functor, by value).  A workgroup bins kBinTile consecutive rows
// into LDS lists (wave-aggregated LDS appends) and appends each list with one global atomic: one per bin per 2048 rows, not
// per wave (same-address atomics serialise).  A hub row takes ceil(len / kSeg) consecutive segment slots (few rows: one
// atomic each).  ctr[0 .. 2]: the lists' cursors.
constexpr int kBinTile = kBlock * 8;
template <int kShortMax, int kSeg, typename Len>
static __global__ __launch_bounds__(kBlock) void row_bin_kernel(Len len_of, Index m, Index* __restrict__ l_short, Index* __restrict__ l_wave,
                                                                Index* __restrict__ seg_row, Index* __restrict__ seg_k,
                                                                unsigned int* __restrict__ ctr) {
  __shared__ Index s_list[2][kBinTile];
  __shared__ unsigned int s_cnt[2], s_base[2];
  const int lane = lane_id();
  for (long long tile = (long long)blockIdx.x * kBinTile; tile < m; tile += (long long)gridDim.x * kBinTile) {
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int x = threadIdx.x - lane; x < kBinTile; x += kBlock) {   // wave-uniform: x is the wave's first row of the step
      const long long i = tile + x + lane;
      int bin = -1;
      long long len = 0;
      if (i < m) {
        len = len_of(i);
        bin = row_bin_of<kShortMax, kSeg>(len);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const unsigned long long mask = __ballot(bin == b);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        unsigned int at = 0;
        if (lane == leader) at = atomicAdd(&s_cnt[b], (unsigned int)__popcll(mask));
        at = (unsigned int)__shfl((int)at, leader, kWave);
        if (bin == b) s_list[b][at + __popcll(mask & ((1ull << lane) - 1ull))] = (Index)i;
      }
      if (bin == 2) {
        const Index nseg = (Index)((len + kSeg - 1) / kSeg);
        const unsigned int at = atomicAdd(&ctr[2], (unsigned int)nseg);
        for (Index k = 0; k < nseg; ++k) { seg_row[at + k] = (Index)i; seg_k[at + k] = k; }
      }
    }
    __syncthreads();
    if (threadIdx.x < 2) s_base[threadIdx.x] = s_cnt[threadIdx.x] ? atomicAdd(&ctr[threadIdx.x], s_cnt[threadIdx.x]) : 0u;
    __syncthreads();
    for (int b = 0; b < 2; ++b) {
      Index* out = (b == 0 ? l_short : l_wave) + s_base[b];
      for (unsigned int j = threadIdx.x; j < s_cnt[b]; j += kBlock) out[j] = s_list[b][j];
    }
    __syncthreads();
  }
}

// a length pass sizes the lists before they exist: every thread adds its rows with row_len_add and the kernel ends with
// row_len_totals.  tot[0 .. 2]: short rows, wave rows, hub segments; tot[3] is the op's own sum.
struct RowLenSums {
  unsigned int n_short = 0, n_wave = 0;
  unsigned long long n_seg = 0, n_own = 0;
};
template <int kShortMax, int kSeg>
__device__ inline void row_len_add(RowLenSums& s, long long len) {
  const int bin = row_bin_of<kShortMax, kSeg>(len);
  s.n_short += bin == 0;
  s.n_wave += bin == 1;
  if (bin == 2) s.n_seg += (unsigned long long)((len + kSeg - 1) / kSeg);
}
__device__ inline void row_len_totals(RowLenSums s, unsigned long long* __restrict__ tot) {
  s.n_short = wave_sum_u32(s.n_short);
  s.n_wave = wave_sum_u32(s.n_wave);
  s.n_seg = wave_sum_u64(s.n_seg);
  s.n_own = wave_sum_u64(s.n_own);
  if (lane_id() == 0) {
    if (s.n_short) atomicAdd(&tot[0], (unsigned long long)s.n_short);
    if (s.n_wave) atomicAdd(&tot[1], (unsigned long long)s.n_wave);
    if (s.n_seg) atomicAdd(&tot[2], s.n_seg);
    if (s.n_own) atomicAdd(&tot[3], s.n_own);
  }
}

// the 64-bit total of the rows' counts and of nseg segments' counts (the u32 scan wraps above 2^32); nseg = 0: rows only
static __global__ __launch_bounds__(kBlock) void count_total_kernel(const unsigned int* __restrict__ counts, Index m,
                                                                    const unsigned int* __restrict__ seg_cnt, Index nseg,
                                                                    unsigned long long* __restrict__ total) {
  unsigned long long acc = 0;
  const long long stride = (long long)gridDim.x * kBlock;
  const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
  for (long long i = first; i < m; i += stride) acc += counts[i];
  for (long long i = first; i < nseg; i += stride) acc += seg_cnt[i];
  acc = wave_sum_u64(acc);
  if (lane_id() == 0 && acc) atomicAdd(total, acc);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// a grid of one block per per_block items, at most 16384 (the kernels stride) and at least one
inline int capped_grid(long long items, int per_block) {
  const long long b = (items + per_block - 1) / per_block;
  return b > 16384 ? 16384 : (int)(b < 1 ? 1 : b);
}
// the bits a radix sort visits for indices below dim
inline int index_bits(Index dim) {
  int b = 1;
  while (b < 31 && ((long long)1 << b) < (long long)dim) ++b;
  return b;
}

// the bins of one call.  The head is 64 bytes: [4] 64-bit sizes of a length pass, [3] list cursors, the 64-bit total.
struct RowBins {
  EwmBuf head, work;                                     // (head stays empty when it is the front of work)
  unsigned long long* d_tot = nullptr;
  unsigned int* d_ctr = nullptr;
  unsigned long long* d_total = nullptr;
  Index *l_short = nullptr, *l_wave = nullptr, *seg_row = nullptr, *seg_k = nullptr;
  unsigned int *seg_cnt = nullptr, *scan = nullptr;
  unsigned int nbin[3] = {0, 0, 0};                      // short rows, wave rows, hub segments
  unsigned long long own = 0;                            // tot[3] of the length pass
};

inline void row_bins_set_head(RowBins* b, void* p) {
  b->d_tot = (unsigned long long*)p;
  b->d_ctr = (unsigned int*)(b->d_tot + 4);
  b->d_total = b->d_tot + 6;
}
inline grb_info row_bins_zero_head(RowBins* b, hipStream_t s) {
  GRB_HIP_TRY(hipMemsetAsync(b->d_tot, 0, 64, s));
  return GRB_SUCCESS;
}
// the head on its own, zeroed: a length pass runs before the lists can be sized
inline grb_info row_bins_head(RowBins* b, hipStream_t s) {
  GRB_TRY(ewm_alloc(&b->head, 64));
  row_bins_set_head(b, b->head.p);
  return row_bins_zero_head(b, s);
}
// the lists for the given capacities and scan scratch for scan_len elements, in one allocation; without a head yet, the
// head is its first 64 bytes (not zeroed here)
inline grb_info row_bins_carve(RowBins* b, size_t cap_short, size_t cap_wave, size_t cap_seg, size_t scan_len) {
  const size_t front = b->d_tot ? 0 : 64;
  GRB_TRY(ewm_alloc(&b->work, front + 4 * (cap_short + cap_wave + 3 * cap_seg + 1) + device_scan_u32_scratch((long long)scan_len)));
  if (front) row_bins_set_head(b, b->work.p);
  b->l_short = (Index*)((char*)b->work.p + front);
  b->l_wave = b->l_short + cap_short;
  b->seg_row = b->l_wave + cap_wave;
  b->seg_k = b->seg_row + cap_seg;
  b->seg_cnt = (unsigned int*)(b->seg_k + cap_seg);
  b->scan = b->seg_cnt + cap_seg + 1;
  return GRB_SUCCESS;
}
// after a length pass over m rows: its sizes read back, the lists carved for exactly that, the segments' counts zeroed
inline grb_info row_bins_sized(RowBins* b, Index m, hipStream_t s) {
  unsigned long long tot[4] = {0, 0, 0, 0};
  if (m > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(tot, b->d_tot, 32, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  if (tot[2] > (unsigned long long)INT32_MAX) return GRB_OUT_OF_MEMORY;   // (the segment lists are indexed in 32 bits)
  for (int k = 0; k < 3; ++k) b->nbin[k] = (unsigned int)tot[k];
  b->own = tot[3];
  const size_t nseg = b->nbin[2];
  GRB_TRY(row_bins_carve(b, b->nbin[0], b->nbin[1], nseg, ((size_t)m > nseg ? (size_t)m : nseg) + 1));
  GRB_HIP_TRY(hipMemsetAsync(b->seg_cnt, 0, 4 * (nseg + 1), s));
  return GRB_SUCCESS;
}
// the lists filled from the rows' lengths
template <int kShortMax, int kSeg, typename Len>
inline grb_info row_bins_fill(const RowBins& b, Len len_of, Index m, hipStream_t s) {
  hipLaunchKernelGGL((row_bin_kernel<kShortMax, kSeg, Len>), dim3(stream_grid(m, kBinTile)), dim3(kBlock), 0, s, len_of, m, b.l_short, b.l_wave,
                     b.seg_row, b.seg_k, b.d_ctr);
  GRB_HIP_TRY(hipGetLastError());
  return GRB_SUCCESS;
}

// f(IntTag<G>, grid, items, seg_k, n) for the bins that are not empty, in the order short, wave, hub: G lanes per item
// (kShortLanes or kWave), seg_k == nullptr but for the hub bin's segments
template <int kShortLanes, typename F>
inline grb_info for_each_bin(const RowBins& b, F f) {
  const Index* none = nullptr;
  if (b.nbin[0]) f(IntTag<kShortLanes>{}, capped_grid(b.nbin[0], kBlock / kShortLanes), (const Index*)b.l_short, none, (Index)b.nbin[0]);
  if (b.nbin[1]) f(IntTag<kWave>{}, capped_grid(b.nbin[1], kWavesPerBlock), (const Index*)b.l_wave, none, (Index)b.nbin[1]);
  if (b.nbin[2]) f(IntTag<kWave>{}, capped_grid(b.nbin[2], kWavesPerBlock), (const Index*)b.seg_row, (const Index*)b.seg_k, (Index)b.nbin[2]);
  GRB_HIP_TRY(hipGetLastError());
  return GRB_SUCCESS;
}

// the symbolic pass's counts -> out->nnz: their total in 64 bits (with the segments' counts where the rows' do not hold them
// yet), GRB_OUT_OF_MEMORY above INT32_MAX (grb_index is 32 bits; nothing of C's entries is allocated yet: C keeps what it held)
inline grb_info row_bins_total(const RowBins& b, const unsigned int* counts, Index m, bool with_segs, hipStream_t s, Side* out) {
  unsigned long long total = 0;
  if (m > 0) {
    const Index nseg = with_segs ? (Index)b.nbin[2] : 0;
    const long long items = with_segs ? (long long)(m > nseg ? m : nseg) + 1 : (long long)m;
    hipLaunchKernelGGL(count_total_kernel, dim3(stream_grid(items, kBlock * 8)), dim3(kBlock), 0, s, counts, m,
                       (const unsigned int*)b.seg_cnt, nseg, b.d_total);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(&total, b.d_total, 8, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  if (total > (unsigned long long)INT32_MAX) return GRB_OUT_OF_MEMORY;
  out->nnz = (Index)total;
  return GRB_SUCCESS;
}
// C's entries: max(nnz, 1) columns and values
inline grb_info side_alloc_entries(Side* out) {
  const size_t cap = (size_t)(out->nnz > 0 ? out->nnz : 1);
  GRB_TRY(ewm_alloc(&out->ind, 4 * cap));
  return ewm_alloc(&out->val, 4 * cap);
}
// counts (out->ptr) -> row pointers, the hub segments' counts -> offsets, the host copy of the pointers, and C's entries
// (entries = false: the caller allocates them)
inline grb_info row_bins_pointers(const RowBins& b, Index m, Side* out, bool entries = true) {
  unsigned int* counts = (unsigned int*)out->ptr.p;
  GRB_TRY(device_exclusive_scan_u32_in(counts, (long long)m + 1, b.scan));
  if (b.nbin[2]) GRB_TRY(device_exclusive_scan_u32_in(b.seg_cnt, (long long)b.nbin[2] + 1, b.scan));
  out->h_ptr.resize((size_t)m + 1);
  GRB_HIP_TRY(hipMemcpy(out->h_ptr.data(), counts, 4 * ((size_t)m + 1), hipMemcpyDeviceToHost));
  return entries ? side_alloc_entries(out) : GRB_SUCCESS;
}

}  // namespace grb
