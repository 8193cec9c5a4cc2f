// sample.hip -- drawing from a graph on the device: grb_random_walk and grb_sample_neighbors.  The contracts are the comment
// in include/grb_hip.h and DESIGN.md 5.4t; the reference has no such drivers (graphblas/algorithm/), the definitions are this
// project's own.  The randomness is counter-based: every draw is a pure function of (seed, who, when),
//   draw(seed, a, b) = mix(mix(mix((seed + 0x9e3779b9) ^ a) + b) ^ seed),   pick(r, m) = (u64(r) * m) >> 32,
// mix = graph_common.hpp's hash_mix32, so the result does not depend on the schedule or the number of CUs and the tests
// compare bits.  Plain launches, no grid barrier, no floating-point arithmetic that decides anything.
//
// Walks.  sm_walk_kernel: a lane a walker, all `length` steps in registers; a step is draw(seed, w, t), the row's two
//   pointers and one index load (uniform), or a binary search in the row's prefix sums and one index load (weighted).  The
//   walker-major stores are plain (a wave's 64 walkers write 64 different lines a step; staging them has not been measured:
//   docs/experiments.md R30).  Steps and dead ends are counted per lane, summed per wave, two 64-bit integer atomics a wave.
//   Weighted mode first builds pre[p] = the inclusive prefix sum of the weights of p's row up to p (u32, 4 bytes an entry,
//   allocated and freed inside the call) in sm_prefix_kernel, rows dealt by length as in msf.hip and matching.hip:
//     up to kSmLaneLen entries   a lane, serially
//     up to kSmWaveLen           a wave: the entries in front of the first 16-byte boundary, then a quad of values a lane and
//                                step (one 16-byte load, one 16-byte store of four prefix sums), then the entries behind
//     longer                     the workgroup, the same walk with the waves' totals through LDS
//   The same pass checks the weights (grb_louvain's rule) and the row sums (<= 2^31 - 1) into a flag word the host reads
//   before the walk starts.  Sums run in 64 bits so that no wrap hides an overflow.
//
// Sampling.  C's row k is row seeds[k] of A whole when its length d <= fanout, else the fanout entries with the smallest
//   key(p) = draw(seed, k, p).  Row lengths min(d, fanout) are known beforehand: sn_len_kernel writes them, the library's scan
//   makes C's pointers, no counting pass.  Keys are recomputed, never stored in memory.  T = the fanout-th smallest key of a
//   row is found by a 32-step BISECTION on count(key <= mid) (chosen over a radix select: no histogram, no LDS for a lane's
//   or a wave's row, and the count is a ballot and a popcount; the two have not been measured against each other); then one
//   pass keeps the entries with key <= T, compacted in stored order by ballot prefix.  Exactly fanout survive: for fixed
//   (seed, k) the key is a bijection of p.  sn_rows_kernel deals the rows by d:
//     up to kSnLaneLen entries   a lane: its keys in registers, an entry is kept when fewer than fanout keys are below its own
//     up to kSnWaveLen           a wave: kSnWaveLen / 64 keys a lane in registers, computed once, bisected by ballots
//     longer                     the workgroup, looping over the row: keys recomputed in every bisection step, the count
//                                through LDS
//   C's CSC is the transpose of the CSR just made (transpose_side, the path behind grb_transpose), as in contract.hip.
#include <climits>

#include "graph_common.hpp"

namespace grb {

constexpr int kSmLaneLen = 8;                            // the prefix pass: a row of up to this many entries: one lane
constexpr int kSmWaveLen = 2048;                         // ... a wave; longer: the workgroup (msf.hip's and matching.hip's pair)
constexpr int kSnLaneLen = 8;                            // sampling: a row of up to this many entries: one lane
constexpr int kSnKeys = 8;                               // keys a lane of a wave's row holds in registers
constexpr int kSnWaveLen = kWave * kSnKeys;              // ... a wave (512); longer: the workgroup
enum { kSmBadWeight = 1u, kSmBadSum = 2u };
// the call's record on the device (64-bit words, zero before the first kernel)
enum { kSmSteps = 0, kSmDead, kSmFlag, kSnEntries, kSnFull, kSmRecWords = 8 };

__device__ __forceinline__ unsigned sm_draw(unsigned seed, unsigned a, unsigned b) {
  return hash_mix32(hash_mix32(hash_mix32((seed + 0x9e3779b9u) ^ a) + b) ^ seed);
}
__device__ __forceinline__ unsigned sm_pick(unsigned r, unsigned m) { return (unsigned)(((unsigned long long)r * (unsigned long long)m) >> 32); }

// ---- the weights' prefix sums ------------------------------------------------------------------------------------------------
// the weight of stored bits b (grb_louvain's rule); bad: it is none
__device__ __forceinline__ unsigned sm_weight(unsigned b, int f32, bool& bad) {
  if (f32) {
    const float f = __uint_as_float(weight_canon(b, 1));
    const bool ok = f >= 0.f && f <= 16777216.f && f == truncf(f);           // (a NaN fails the first)
    bad |= !ok;
    return ok ? (unsigned)f : 0u;
  }
  bad |= (int)b < 0;
  return (int)b < 0 ? 0u : b;
}

// the group's inclusive scan of x and its total: a wave (kWide = false) or the kBlock-thread workgroup, through s_tot
template <bool kWide>
__device__ __forceinline__ unsigned long long sm_group_scan(unsigned long long x, unsigned long long* s_tot, unsigned long long& total) {
  unsigned long long incl = wave_incl_scan_u64(x);
  const unsigned long long wtot = __shfl(incl, kWave - 1, kWave);
  if (!kWide) {
    total = wtot;
    return incl;
  }
  __syncthreads();                                                           // (the totals of the step before have been read)
  if (lane_id() == kWave - 1) s_tot[wave_id()] = wtot;
  __syncthreads();
  total = 0;
  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (w < wave_id()) incl += s_tot[w];
    total += s_tot[w];
  }
  return incl;
}

// pre[b .. e) of one row by a group of kThreads threads, thread t; every thread of the group calls it with the same row
template <bool kWide>
__device__ __forceinline__ void sm_prefix_row(const unsigned* __restrict__ val, unsigned* __restrict__ pre, Index b, Index e, int f32, int t,
                                              unsigned long long* s_tot, bool& bad, bool& over) {
  constexpr int kThreads = kWide ? kBlock : kWave;
  const QuadSpan s = quad_span((const Index*)val, b, e);                     // (4-byte entries: the same split)
  unsigned long long carry = 0, total;
  {                                                                          // the entries in front of the first quad
    const bool in = t < s.nh;
    const unsigned long long x = in ? sm_weight(val[b + t], f32, bad) : 0u;
    const unsigned long long incl = sm_group_scan<kWide>(x, s_tot, total);
    if (in) pre[b + t] = (unsigned)incl;
    carry = total;
  }
  for (Index q0 = 0; q0 < s.nq; q0 += kThreads) {                            // a quad a thread and step
    const Index q = q0 + t;
    const bool in = q < s.nq;
    const Index at = s.b4 + 4 * q;
    uint4 w = {0u, 0u, 0u, 0u};
    if (in) {
      const uint4 raw = *reinterpret_cast<const uint4*>(val + at);
      w.x = sm_weight(raw.x, f32, bad);
      w.y = sm_weight(raw.y, f32, bad);
      w.z = sm_weight(raw.z, f32, bad);
      w.w = sm_weight(raw.w, f32, bad);
    }
    const unsigned long long mine = (unsigned long long)w.x + w.y + w.z + w.w;
    const unsigned long long incl = sm_group_scan<kWide>(mine, s_tot, total);
    if (in) {
      const unsigned long long base = carry + incl - mine;
      uint4 o;
      o.x = (unsigned)(base + w.x);
      o.y = (unsigned)(base + w.x + w.y);
      o.z = (unsigned)(base + w.x + w.y + w.z);
      o.w = (unsigned)(base + mine);
      *reinterpret_cast<uint4*>(pre + at) = o;                               // (pre begins at val's offset inside a 16-byte line)
    }
    carry += total;
  }
  {                                                                          // the entries behind the last quad
    const Index nt = e - s.te;
    const bool in = t < nt;
    const unsigned long long x = in ? sm_weight(val[s.te + t], f32, bad) : 0u;
    const unsigned long long incl = sm_group_scan<kWide>(x, s_tot, total);
    if (in) pre[s.te + t] = (unsigned)(carry + incl);
    carry += total;
  }
  over |= carry > (unsigned long long)INT32_MAX;
}

__global__ __launch_bounds__(kBlock) void sm_prefix_kernel(const Index* __restrict__ ptr, const unsigned* __restrict__ val, long long n, int f32,
                                                           unsigned* __restrict__ pre, unsigned long long* __restrict__ rec) {
  __shared__ Index s_big[kBlock];
  __shared__ int s_nbig;
  __shared__ unsigned long long s_tot[kWavesPerBlock];
  const int tid = threadIdx.x, lane = lane_id();
  bool bad = false, over = false;
  for (long long base = (long long)blockIdx.x * kBlock; base < n; base += (long long)gridDim.x * kBlock) {
    if (tid == 0) s_nbig = 0;
    __syncthreads();
    const long long i = base + tid;
    Index v = 0, b = 0, e = 0;
    if (i < n) {
      v = (Index)i;
      b = ptr[v];
      e = ptr[v + 1];
    }
    const Index len = e > b ? e - b : 0;
    if (len > kSmWaveLen) s_big[atomicAdd(&s_nbig, 1)] = v;                  // (at most one a thread: room for all)
    if (len > 0 && len <= kSmLaneLen) {                                      // ---- a lane a row
      unsigned long long sum = 0;
      for (Index p = b; p < e; ++p) {
        sum += sm_weight(val[p], f32, bad);
        pre[p] = (unsigned)sum;
      }
      over |= sum > (unsigned long long)INT32_MAX;
    }
    unsigned long long mids = __ballot(len > kSmLaneLen && len <= kSmWaveLen);
    while (mids) {                                                           // ---- a wave a row
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wb = (Index)__builtin_amdgcn_readlane((int)b, l);
      const Index we = (Index)__builtin_amdgcn_readlane((int)e, l);
      sm_prefix_row<false>(val, pre, wb, we, f32, lane, nullptr, bad, over);
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int r = 0; r < nbig; ++r) {                                         // ---- the workgroup a row
      const Index wv = s_big[r];
      sm_prefix_row<true>(val, pre, ptr[wv], ptr[wv + 1], f32, tid, s_tot, bad, over);
    }
    __syncthreads();
  }
  const unsigned f = (bad ? (unsigned)kSmBadWeight : 0u) | (over ? (unsigned)kSmBadSum : 0u);
  if (f) atomicOr(&rec[kSmFlag], (unsigned long long)f);
}

// ---- the walks -----------------------------------------------------------------------------------------------------------------
// out[w * (length + 1) + t] = walker w's vertex after t steps, -1 behind a dead end.  starts == nullptr: walker w starts at w.
template <bool kWeighted>
__global__ __launch_bounds__(kBlock) void sm_walk_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, const unsigned* __restrict__ pre,
                                                         Index n, const Index* __restrict__ starts, long long ns, int length, unsigned seed,
                                                         int* __restrict__ out, unsigned long long* __restrict__ rec) {
  unsigned long long steps = 0;
  unsigned dead = 0;
  for (long long w = (long long)blockIdx.x * kBlock + threadIdx.x; w < ns; w += (long long)gridDim.x * kBlock) {
    int* const row = out + w * ((long long)length + 1);
    Index v = starts ? starts[w] : (Index)w;
    row[0] = v;
    int t = 0;
    for (; t < length; ++t) {
      const Index b = ptr ? ptr[v] : 0, e = ptr ? ptr[v + 1] : 0;           // (ptr == nullptr: a matrix without entries)
      if (e <= b) break;
      const unsigned r = sm_draw(seed, (unsigned)w, (unsigned)t);
      Index p;
      if (kWeighted) {
        const unsigned S = pre[e - 1];
        if (S == 0u) break;
        const unsigned x = sm_pick(r, S);
        Index lo = b, hi = e - 1;                        // the first p with pre[p] > x; pre[e - 1] = S > x
        while (lo < hi) {
          const Index mid = lo + ((hi - lo) >> 1);
          if (pre[mid] > x) hi = mid; else lo = mid + 1;
        }
        p = lo;
      } else {
        p = b + (Index)sm_pick(r, (unsigned)(e - b));
      }
      const Index u = ind[p];
      if ((unsigned)u >= (unsigned)n) break;             // (never: a built matrix has no such column)
      v = u;
      row[t + 1] = v;
    }
    steps += (unsigned long long)t;
    if (t < length) {
      ++dead;
      for (int q = t + 1; q <= length; ++q) row[q] = -1;
    }
  }
  steps = wave_sum_u64(steps);
  dead = wave_sum_u32(dead);
  if (lane_id() == 0) {
    if (steps) atomicAdd(&rec[kSmSteps], steps);
    if (dead) atomicAdd(&rec[kSmDead], (unsigned long long)dead);
  }
}

// ---- sampling ------------------------------------------------------------------------------------------------------------------
// counts[k] = min(d(seeds[k]), fanout), counts[ns] = 0; their 64-bit total and the rows copied whole
__global__ __launch_bounds__(kBlock) void sn_len_kernel(const Index* __restrict__ ptr, const Index* __restrict__ seeds, long long ns, int fanout,
                                                        unsigned* __restrict__ counts, unsigned long long* __restrict__ rec) {
  unsigned long long total = 0;
  unsigned full = 0;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k <= ns; k += (long long)gridDim.x * kBlock) {
    unsigned c = 0;
    if (k < ns) {
      const Index r = seeds[k];
      const Index d = ptr[r + 1] - ptr[r];
      c = d > 0 ? (unsigned)(d < fanout ? d : fanout) : 0u;
      full += d <= fanout ? 1u : 0u;
      total += c;
    }
    counts[k] = c;
  }
  total = wave_sum_u64(total);
  full = wave_sum_u32(full);
  if (lane_id() == 0) {
    if (total) atomicAdd(&rec[kSnEntries], total);
    if (full) atomicAdd(&rec[kSnFull], (unsigned long long)full);
  }
}

// the workgroup's sum of c (kBlock threads, every thread calls it), in every thread
__device__ __forceinline__ unsigned sn_block_sum(unsigned c, unsigned* s_cnt) {
  c = wave_sum_u32(c);
  __syncthreads();                                                           // (the sums of the step before have been read)
  if (lane_id() == 0) s_cnt[wave_id()] = c;
  __syncthreads();
  unsigned t = 0;
  for (int w = 0; w < kWavesPerBlock; ++w) t += s_cnt[w];
  return t;
}

__global__ __launch_bounds__(kBlock) void sn_rows_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, const unsigned* __restrict__ val,
                                                         const Index* __restrict__ seeds, long long ns, int fanout, unsigned seed,
                                                         const Index* __restrict__ c_ptr, Index* __restrict__ c_ind, unsigned* __restrict__ c_val) {
  __shared__ Index s_big[kBlock];                                            // list positions k
  __shared__ int s_nbig;
  __shared__ unsigned s_cnt[kWavesPerBlock];
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long base = (long long)blockIdx.x * kBlock; base < ns; base += (long long)gridDim.x * kBlock) {
    if (tid == 0) s_nbig = 0;
    __syncthreads();
    const long long i = base + tid;
    Index k = 0, b = 0, e = 0, out = 0;
    if (i < ns) {
      k = (Index)i;
      const Index r = seeds[k];
      b = ptr[r];
      e = ptr[r + 1];
      out = c_ptr[k];
    }
    const Index len = e > b ? e - b : 0;
    if (len > kSnWaveLen) s_big[atomicAdd(&s_nbig, 1)] = k;                  // (at most one a thread: room for all)
    if (len > 0 && len <= kSnLaneLen) {                                      // ---- a lane a row
      if (len <= fanout) {
        for (Index j = 0; j < len; ++j) {
          c_ind[out + j] = ind[b + j];
          c_val[out + j] = val[b + j];
        }
      } else {
        unsigned key[kSnLaneLen];
#pragma unroll
        for (int j = 0; j < kSnLaneLen; ++j) key[j] = j < len ? sm_draw(seed, (unsigned)k, (unsigned)j) : 0xffffffffu;
        Index o = out;
#pragma unroll
        for (int j = 0; j < kSnLaneLen; ++j) {
          int rank = 0;
#pragma unroll
          for (int q = 0; q < kSnLaneLen; ++q) rank += q < len && key[q] < key[j] ? 1 : 0;
          if (j < len && rank < fanout) {
            c_ind[o] = ind[b + j];
            c_val[o] = val[b + j];
            ++o;
          }
        }
      }
    }
    unsigned long long mids = __ballot(len > kSnLaneLen && len <= kSnWaveLen);
    while (mids) {                                                           // ---- a wave a row
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const unsigned wk = (unsigned)__builtin_amdgcn_readlane((int)k, l);
      const Index wb = (Index)__builtin_amdgcn_readlane((int)b, l);
      const Index wlen = (Index)__builtin_amdgcn_readlane((int)len, l);
      Index wout = (Index)__builtin_amdgcn_readlane((int)out, l);
      if (wlen <= fanout) {
        for (Index p = lane; p < wlen; p += kWave) {
          c_ind[wout + p] = ind[wb + p];
          c_val[wout + p] = val[wb + p];
        }
        continue;
      }
      unsigned key[kSnKeys];
#pragma unroll
      for (int j = 0; j < kSnKeys; ++j) key[j] = sm_draw(seed, wk, (unsigned)(j * kWave + lane));
      unsigned lo = 0u, hi = 0xffffffffu;                                    // the smallest T with count(key <= T) >= fanout
      while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        int c = 0;
#pragma unroll
        for (int j = 0; j < kSnKeys; ++j) c += __popcll(__ballot(j * kWave + lane < wlen && key[j] <= mid));
        if (c >= fanout) hi = mid; else lo = mid + 1u;
      }
#pragma unroll
      for (int j = 0; j < kSnKeys; ++j) {
        const Index p = j * kWave + lane;
        const bool keep = p < wlen && key[j] <= lo;
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const Index o = wout + (Index)__popcll(m & below);
          c_ind[o] = ind[wb + p];
          c_val[o] = val[wb + p];
        }
        wout += (Index)__popcll(m);
      }
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int r = 0; r < nbig; ++r) {                                         // ---- the workgroup a row, looping over it
      const unsigned wk = (unsigned)s_big[r];
      const Index row = seeds[wk];
      const Index wb = ptr[row], wlen = ptr[row + 1] - wb;
      Index wout = c_ptr[wk];
      if (wlen <= fanout) {
        for (Index p = tid; p < wlen; p += kBlock) {
          c_ind[wout + p] = ind[wb + p];
          c_val[wout + p] = val[wb + p];
        }
        continue;
      }
      unsigned lo = 0u, hi = 0xffffffffu;
      while (lo < hi) {                                                      // (lo and hi are the same in every thread)
        const unsigned mid = lo + ((hi - lo) >> 1);
        unsigned c = 0;
        for (Index p = tid; p < wlen; p += kBlock) c += sm_draw(seed, wk, (unsigned)p) <= mid ? 1u : 0u;
        if (sn_block_sum(c, s_cnt) >= (unsigned)fanout) hi = mid; else lo = mid + 1u;
      }
      for (Index p0 = 0; p0 < wlen; p0 += kBlock) {
        const Index p = p0 + tid;
        const bool keep = p < wlen && sm_draw(seed, wk, (unsigned)p) <= lo;
        const unsigned long long m = __ballot(keep);
        __syncthreads();
        if (lane == 0) s_cnt[wave] = (unsigned)__popcll(m);
        __syncthreads();
        Index o = wout + (Index)__popcll(m & below);
        Index all = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) {
          if (w < wave) o += (Index)s_cnt[w];
          all += (Index)s_cnt[w];
        }
        if (keep) {
          c_ind[o] = ind[wb + p];
          c_val[o] = val[wb + p];
        }
        wout += all;
      }
    }
    __syncthreads();
  }
}

namespace {

grb_info walk_run(grb_vector walks, grb_matrix A, const Index* starts, long long ns, int length, int mode, unsigned seed, grb_walk_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = A->nrows;
  const long long Z = A->csr.ptr ? (long long)A->nvals : 0;
  const long long total = ns * ((long long)length + 1);
  grb_walk_result r = {};
  r.walkers = ns;
  GRB_TRY(dense_out_prepare(walks, (Index)total));       // before anything runs; walks stays as it was until the walk kernel
  if (ns == 0) {
    GRB_TRY(dense_out_commit(walks, nullptr, 0, s));
    if (res) *res = r;
    return GRB_SUCCESS;
  }
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the record, the starts, and in weighted mode the prefix sums
  const bool weighted = mode == GRB_WALK_WEIGHTED && Z > 0;
  const size_t sw = starts ? pad_words((size_t)ns) : 0, pw = weighted ? pad_words((size_t)Z + 8) : 0;
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 256 + 4 * (sw + pw)));
  unsigned long long* d_rec = (unsigned long long*)work.p;
  Index* d_starts = starts ? (Index*)((char*)work.p + 256) : nullptr;
  unsigned* d_pbase = (unsigned*)((char*)work.p + 256) + sw;
  // the prefix sums begin at the same offset inside a 16-byte line as A's values (an adopted array may begin at any 4-byte
  // boundary): a quad of values and the quad of their sums are both aligned
  unsigned* d_pre = weighted ? d_pbase + ((reinterpret_cast<uintptr_t>(A->csr.val) >> 2) & 3u) : nullptr;
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 256, s));
  if (starts) GRB_HIP_TRY(hipMemcpyAsync(d_starts, starts, 4 * (size_t)ns, hipMemcpyHostToDevice, s));
  if (weighted) {
    hipLaunchKernelGGL(sm_prefix_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, A->csr.ptr, (const unsigned*)A->csr.val, (long long)n,
                       A->dtype == GRB_F32 ? 1 : 0, d_pre, d_rec);
    GRB_HIP_TRY(hipGetLastError());
    ++r.launches;
    unsigned long long flag = 0;
    GRB_HIP_TRY(hipMemcpyAsync(&flag, d_rec + kSmFlag, 8, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the check, before walks is written
    if (flag) return GRB_INVALID_VALUE;                  // a weight that is no non-negative integer, or a row sum > 2^31 - 1
  }
  // everything that can fail is behind us: the walk writes walks' own dense storage
  int* out = (int*)walks->d_val;
  if (weighted)
    hipLaunchKernelGGL(sm_walk_kernel<true>, dim3(stream_grid(ns)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, (const unsigned*)d_pre, n,
                       (const Index*)d_starts, ns, length, seed, out, d_rec);
  else                                                   // (a matrix without entries: every start is a dead end)
    hipLaunchKernelGGL(sm_walk_kernel<false>, dim3(stream_grid(ns)), dim3(kBlock), 0, s, (const Index*)(Z > 0 ? A->csr.ptr : nullptr), A->csr.ind, (const unsigned*)nullptr, n,
                       (const Index*)d_starts, ns, length, seed, out, d_rec);
  GRB_HIP_TRY(hipGetLastError());
  ++r.launches;
  unsigned long long h[kSmRecWords];
  GRB_HIP_TRY(hipMemcpyAsync(h, d_rec, sizeof(h), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  walks->vec_type = GRB_DENSE;
  walks->d_nnz = (Index)total;
  r.steps = (int64_t)h[kSmSteps];
  r.dead_ends = (int64_t)h[kSmDead];
  if (res) *res = r;
  return GRB_SUCCESS;
}

grb_info sample_run(grb_matrix C, grb_matrix A, const Index* seeds, Index ns, int fanout, unsigned seed, grb_sample_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index ncols = A->ncols;
  const bool both = C->format != 1;
  grb_sample_result r = {};
  r.rows = ns;
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the record, the seeds, the scan's totals; C's pointers are the scanned counts
  const size_t sw = pad_words((size_t)ns + 1);
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 256 + 4 * sw + pad_bytes(device_scan_u32_scratch((long long)ns + 1))));
  unsigned long long* d_rec = (unsigned long long*)work.p;
  Index* d_seeds = (Index*)((char*)work.p + 256);
  unsigned* d_totals = (unsigned*)(d_seeds + sw);
  Side sr, sc;
  GRB_TRY(ewm_alloc(&sr.ptr, 4 * ((size_t)ns + 1)));
  sr.h_ptr.assign((size_t)ns + 1, 0);
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 256, s));
  long long E = 0;
  unsigned long long h[kSmRecWords] = {};
  if (ns > 0 && A->nvals > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(d_seeds, seeds, 4 * (size_t)ns, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sn_len_kernel, dim3(stream_grid((long long)ns + 1)), dim3(kBlock), 0, s, A->csr.ptr, (const Index*)d_seeds, (long long)ns, fanout,
                       (unsigned*)sr.ptr.p, d_rec);
    GRB_HIP_TRY(hipGetLastError());
    ++r.launches;
    GRB_HIP_TRY(hipMemcpyAsync(h, d_rec, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the call's first read: nvals(C), before anything of C is allocated
    if (h[kSnEntries] > (unsigned long long)INT32_MAX) return GRB_OUT_OF_MEMORY;
    E = (long long)h[kSnEntries];
    GRB_TRY(device_exclusive_scan_u32_async((unsigned*)sr.ptr.p, (long long)ns + 1, d_totals));
    r.launches += 3;
    GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)ns + 1), hipMemcpyDeviceToHost, s));
  } else {                                               // no rows, or an A without entries: every row is empty and "whole"
    GRB_HIP_TRY(hipMemsetAsync(sr.ptr.p, 0, 4 * ((size_t)ns + 1), s));
    h[kSnFull] = (unsigned long long)ns;
  }
  GRB_TRY(ewm_alloc(&sr.ind, 4 * (size_t)(E > 0 ? E : 1)));
  GRB_TRY(ewm_alloc(&sr.val, 4 * (size_t)(E > 0 ? E : 1)));
  sr.nnz = (Index)E;
  if (E > 0) {
    hipLaunchKernelGGL(sn_rows_kernel, dim3(stream_grid(ns)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, (const unsigned*)A->csr.val,
                       (const Index*)d_seeds, (long long)ns, fanout, seed, (const Index*)sr.ptr.p, (Index*)sr.ind.p, (unsigned*)sr.val.p);
    GRB_HIP_TRY(hipGetLastError());
    ++r.launches;
  }
  // ---- the CSC: the transpose of the CSR just made (the path behind grb_transpose)
  if (both) {
    if (E > 0) {
      CsrArrays X;
      X.ptr = (Index*)sr.ptr.p;
      X.ind = (Index*)sr.ind.p;
      X.val = sr.val.p;
      X.n = ns;
      X.nvals = (Index)E;
      GRB_TRY(transpose_side(X, ns, ncols, &sc));
    } else {
      GRB_TRY(ewm_alloc(&sc.ptr, 4 * ((size_t)ncols + 1)));
      GRB_TRY(ewm_alloc(&sc.ind, 4));
      GRB_TRY(ewm_alloc(&sc.val, 4));
      GRB_HIP_TRY(hipMemsetAsync(sc.ptr.p, 0, 4 * ((size_t)ncols + 1), s));
      sc.h_ptr.assign((size_t)ncols + 1, 0);
      sc.nnz = 0;
    }
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  r.entries = (int64_t)E;
  r.full_rows = (int64_t)h[kSnFull];
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches C).  A, which may be C, has
  // been read for the last time
  GRB_TRY(attach(C, &sr, both ? &sc : nullptr));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contracts are the comments in include/grb_hip.h
grb_info grb_random_walk(grb_vector walks, grb_matrix A, const grb_index* starts, int64_t ns, int length, int mode, uint32_t seed,
                         grb_descriptor desc, grb_walk_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!walks || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (!starts) ns = n;
  if (ns < 0 || length < 0 || (mode != GRB_WALK_UNIFORM && mode != GRB_WALK_WEIGHTED)) return GRB_INVALID_VALUE;
  if (A->nrows != A->ncols) return GRB_DIMENSION_MISMATCH;
  if (ns > (int64_t)INT32_MAX || ns * ((int64_t)length + 1) > (int64_t)INT32_MAX) return GRB_INVALID_VALUE;
  if ((int64_t)walks->nsize != ns * ((int64_t)length + 1)) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || walks->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  if (starts)
    for (int64_t w = 0; w < ns; ++w)
      if (starts[w] < 0 || starts[w] >= n) return GRB_INVALID_INDEX;
  if (A->nvals > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return walk_run(walks, A, starts, (long long)ns, length, mode, seed, result);
}

grb_info grb_sample_neighbors(grb_matrix C, grb_matrix A, const grb_index* seeds, grb_index ns, int fanout, uint32_t seed,
                              grb_descriptor desc, grb_sample_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!C || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  if (!seeds && ns > 0) return GRB_NULL_POINTER;
  if (fanout < 1 || ns < 0) return GRB_INVALID_VALUE;
  if (C->nrows != ns || C->ncols != A->ncols) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  for (Index k = 0; k < ns; ++k)
    if (seeds[k] < 0 || seeds[k] >= A->nrows) return GRB_INDEX_OUT_OF_BOUNDS;
  if (A->nvals > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return sample_run(C, A, seeds, ns, fanout, seed, result);
}
