// lcc.hip -- the local clustering coefficient on the device: grb_lcc.  The contract is the comment in include/grb_hip.h; the
// reference has no such driver (graphblas/algorithm/), the definition is Graphalytics' and LAGraph's:
//   N(v) = the vertices joined to v in either direction (a set), d(v) = |N(v)|,
//   num(v) = the stored entries (u, w), u != w, with both ends in N(v),   lcc(v) = num(v) / (d(v) (d(v) - 1)).
//
// With m(v, u) in {1, 2} = how many of (v, u) and (u, v) are stored, num is a property of the triangles of the undirected
// graph: num(a) = the sum of m(b, c) over the triangles {a, b, c}.  So one enumeration serves the directed and the
// undirected case (there m = 2 throughout), and every triangle is met ONCE, as tc_count.hip meets it:
//   S        the working graph, structure only: row v = N(v) ascending, each entry with the bit m - 1 on top of the index
//            (indices are below 2^31).  A wave a vertex: every entry of the CSR row looks itself up in the CSC column and
//            the other way round (both ascending), which gives its place in the merged row; the diagonal is dropped.
//   O        the orientation: O(v) = the entries of S's row v that rank above v by (d, id), at most sqrt(2 entries) of them
//            on a symmetric structure.  Every list starts at a multiple of 16 bytes and is filled up to one with kLcPad.
//   P        per pivot its partners: an edge {v, u} is intersected from the end with the longer list, the PIVOT (the
//            lower-ranked end on a tie); the other end is its partner, dropped when its list is empty.
//   tasks    a pivot and up to kLcChunk[c] of its partners; class 0: pivots with lists of up to kLcWaveLen entries, a wave;
//            class 1: the longer ones, a workgroup.  Counts, one scan, a fill; the kernels read the number of tasks from
//            the device.
//   enum     the pivot's list goes into an LDS hash table, kLcKeys entries at a time (a longer list is taken in slices and
//            the partners are streamed once per slice); the partners' lists go past it 16 bytes a lane: a partner of up
//            to kLcLaneLen entries is walked by ONE lane, 64 partners at a time, a longer one by the wave.  A hit w in the
//            list of partner q is the triangle {p, q, w}: p gets m(q, w) in a register (reduced once per task), w gets
//            m(p, q) in the 32-bit LDS counter beside its slot, q gets m(p, w) in a register, reduced per partner and
//            then added to q's LDS counter if q is in the table (it is whenever q ranks above p and lies in the slice),
//            else to num(q).  The counters are flushed with one 64-bit integer atomicAdd per non-zero slot.  No global
//            atomic per triangle, no floating-point atomic: integer adds commute, so the bits do not depend on the order.
//   final    d (d - 1), the f64 quotient rounded to f32 once, and the record's totals.
// Everything is carved from one allocation before the first kernel; the host reads one record.
#include "graph_common.hpp"

namespace grb {

constexpr unsigned kLcBit = 0x80000000u;                 // m - 1 of an entry
constexpr unsigned kLcIdx = 0x7fffffffu;                 // its vertex
constexpr unsigned kLcPad = 0x7fffffffu;                 // fills a list up to a multiple of four entries: nobody's id
constexpr unsigned kLcEmpty = 0xffffffffu;               // a free slot
constexpr int kLcWaveLen = 256;                          // a pivot's list of up to this many entries: a wave's task
constexpr int kLcWaveSlots = 2 * kLcWaveLen;             // ... and its table, at most half full
constexpr int kLcKeys = 2048;                            // entries of a longer list in the table at a time: a slice
constexpr int kLcSlots = 2 * kLcKeys;                    // (key, counter) pairs of the workgroup's table: 32 KiB
constexpr int kLcLaneLen = 32;                           // a partner's list of up to this many entries: one lane walks it
constexpr int kLcChunk[2] = {256, 1024};                 // partners per task, by class
constexpr int kLcTotals = 64;                            // partial triangle counts (one address would serialise the tasks)
static_assert((kLcWaveSlots & (kLcWaveSlots - 1)) == 0 && (kLcSlots & (kLcSlots - 1)) == 0 && kLcTotals == kWave, "sizes");

// ---- S: the merged rows ---------------------------------------------------------------------------------------------------
// kFill false: sptr[v] = d(v).  kFill true: sptr is scanned and row v of S is written.  cptr == nullptr: rows only, m = 2.
// An entry's place in the merged row = the kept entries of its own list before it + the kept entries of the other list
// below it that are not in both; "in both and below it" is the same set seen from either list, a running count.
template <bool kFill>
__global__ __launch_bounds__(kBlock) void lc_merge_kernel(const Index* __restrict__ rptr, const Index* __restrict__ rind,
                                                          const Index* __restrict__ cptr, const Index* __restrict__ cind, Index n,
                                                          unsigned int* __restrict__ sptr, unsigned int* __restrict__ S) {
  const int lane = lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const Index rb = rptr[v], re = rptr[v + 1];
    const Index cb = cptr ? cptr[v] : 0, ce = cptr ? cptr[v + 1] : 0;
    const Index dr = index_lower_bound(rind, rb, re, (Index)v);             // where the diagonal lies, if stored
    const bool has_r = dr < re && rind[dr] == (Index)v;
    const Index dc = cptr ? index_lower_bound(cind, cb, ce, (Index)v) : 0;
    const bool has_c = cptr && dc < ce && cind[dc] == (Index)v;
    const unsigned base = kFill ? sptr[v] : 0u, room = kFill ? sptr[v + 1] - base : 0u;
    unsigned both = 0;                                                   // entries in both lists, before this step
    for (Index x0 = rb; x0 < re; x0 += kWave) {
      const Index x = x0 + lane;
      const Index u = x < re ? rind[x] : (Index)v;
      const bool keep = x < re && u != (Index)v;
      Index pc = cb;
      bool found = false;
      if (keep && cptr) {
        pc = index_lower_bound(cind, cb, ce, u);
        found = pc < ce && cind[pc] == u;
      }
      const unsigned long long bm = __ballot(found);
      if (kFill && keep) {
        const unsigned pos = (unsigned)(x - rb) - (has_r && dr < x ? 1u : 0u) + (unsigned)(pc - cb) - (has_c && dc < pc ? 1u : 0u) -
                             (both + (unsigned)__popcll(bm & below));
        if (pos < room) S[base + pos] = (unsigned)u | (found || !cptr ? kLcBit : 0u);
      }
      both += (unsigned)__popcll(bm);
    }
    const unsigned nboth = both;
    both = 0;
    for (Index x0 = cb; x0 < ce; x0 += kWave) {
      const Index x = x0 + lane;
      const Index w = x < ce ? cind[x] : (Index)v;
      const bool keep = x < ce && w != (Index)v;
      Index pr = rb;
      bool found = false;
      if (keep) {
        pr = index_lower_bound(rind, rb, re, w);
        found = pr < re && rind[pr] == w;
      }
      const unsigned long long bm = __ballot(found);
      if (kFill && keep && !found) {
        const unsigned pos = (unsigned)(x - cb) - (has_c && dc < x ? 1u : 0u) - (both + (unsigned)__popcll(bm & below)) +
                             (unsigned)(pr - rb) - (has_r && dr < pr ? 1u : 0u);
        if (pos < room) S[base + pos] = (unsigned)w;
      }
      both += (unsigned)__popcll(bm);
    }
    if (!kFill && lane == 0) sptr[v] = (unsigned)(re - rb) - (has_r ? 1u : 0u) + (unsigned)(ce - cb) - (has_c ? 1u : 0u) - nboth;
  }
}

// does u rank above v?  (d, id) ascending; an id outside the matrix ranks nowhere
__device__ __forceinline__ bool lc_above(const unsigned int* __restrict__ sptr, Index n, unsigned u, unsigned v, unsigned dv) {
  if (u >= (unsigned)n) return false;
  const unsigned du = sptr[u + 1] - sptr[u];
  return du > dv || (du == dv && u > v);
}

// ---- O: the lists' lengths, then the lists and every pivot's number of partners ------------------------------------------
__global__ __launch_bounds__(kBlock) void lc_olen_kernel(const unsigned int* __restrict__ sptr, const unsigned int* __restrict__ S, Index n,
                                                         unsigned int* __restrict__ olen, unsigned int* __restrict__ optr) {
  const int lane = lane_id();
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const unsigned b = sptr[v], e = sptr[v + 1];
    unsigned cnt = 0;
    for (unsigned x = b + lane; x < e; x += kWave) cnt += lc_above(sptr, n, S[x] & kLcIdx, (unsigned)v, e - b) ? 1u : 0u;
    cnt = wave_sum_u32(cnt);
    if (lane == 0) { olen[v] = cnt; optr[v] = (cnt + 3u) & ~3u; }
  }
}

// who intersects the edge {v, u}, u in O(v): the end with the longer list is the pivot, v on a tie
__device__ __forceinline__ void lc_roles(unsigned v, unsigned u, const unsigned int* __restrict__ olen, unsigned* pivot, unsigned* partner,
                                         unsigned* plen) {
  const unsigned lv = olen[v], lu = olen[u];
  const bool u_is_pivot = lu > lv;
  *pivot = u_is_pivot ? u : v;
  *partner = u_is_pivot ? v : u;
  *plen = u_is_pivot ? lv : lu;
}

__global__ __launch_bounds__(kBlock) void lc_ofill_kernel(const unsigned int* __restrict__ sptr, const unsigned int* __restrict__ S, Index n,
                                                          const unsigned int* __restrict__ olen, const unsigned int* __restrict__ optr,
                                                          unsigned int* __restrict__ O, unsigned int* __restrict__ pcnt) {
  const int lane = lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const unsigned b = sptr[v], e = sptr[v + 1], base = optr[v], len = olen[v];
    unsigned run = 0;
    for (unsigned x0 = b; x0 < e; x0 += kWave) {
      const unsigned x = x0 + lane;
      const unsigned ent = x < e ? S[x] : 0u;
      const bool above = x < e && lc_above(sptr, n, ent & kLcIdx, (unsigned)v, e - b);
      const unsigned long long bm = __ballot(above);
      if (above) {
        const unsigned at = run + (unsigned)__popcll(bm & below);
        if (at < len) O[base + at] = ent;
        unsigned pivot, partner, plen;
        lc_roles((unsigned)v, ent & kLcIdx, olen, &pivot, &partner, &plen);
        if (plen > 0u) atomicAdd(&pcnt[pivot], 1u);
      }
      run += (unsigned)__popcll(bm);
    }
    for (unsigned k = len + lane; k < ((len + 3u) & ~3u); k += kWave) O[base + k] = kLcPad;
  }
}

// the partners themselves, in whatever order the atomics hand out (pcur starts as a copy of pptr)
__global__ __launch_bounds__(kBlock) void lc_pfill_kernel(Index n, const unsigned int* __restrict__ olen, const unsigned int* __restrict__ optr,
                                                          const unsigned int* __restrict__ O, const unsigned int* __restrict__ pptr,
                                                          unsigned int* __restrict__ pcur, unsigned int* __restrict__ P) {
  const int lane = lane_id();
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const unsigned base = optr[v], len = olen[v];
    for (unsigned k = lane; k < len; k += kWave) {
      const unsigned ent = O[base + k];
      unsigned pivot, partner, plen;
      lc_roles((unsigned)v, ent & kLcIdx, olen, &pivot, &partner, &plen);
      if (plen > 0u) {
        const unsigned at = atomicAdd(&pcur[pivot], 1u);
        if (at < pptr[pivot + 1]) P[at] = partner | (ent & kLcBit);
      }
    }
  }
}

// ---- the task lists -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lc_class(unsigned len, unsigned np) { return np == 0u ? -1 : len <= (unsigned)kLcWaveLen ? 0 : 1; }
__global__ __launch_bounds__(kBlock) void lc_task_count_kernel(const unsigned int* __restrict__ olen, const unsigned int* __restrict__ pptr, Index n,
                                                               unsigned int* __restrict__ c0, unsigned int* __restrict__ c1) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const unsigned np = pptr[p + 1] - pptr[p];
  const int c = lc_class(olen[p], np);
  c0[p] = c == 0 ? (np + kLcChunk[0] - 1) / kLcChunk[0] : 0u;
  c1[p] = c == 1 ? (np + kLcChunk[1] - 1) / kLcChunk[1] : 0u;
}
// {pivot, first partner, partners, -}
__global__ __launch_bounds__(kBlock) void lc_task_fill_kernel(const unsigned int* __restrict__ olen, const unsigned int* __restrict__ pptr, Index n,
                                                              const unsigned int* __restrict__ c0, const unsigned int* __restrict__ c1,
                                                              int4* __restrict__ t0, int4* __restrict__ t1, unsigned room0, unsigned room1) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const unsigned first = pptr[p], np = pptr[p + 1] - first;
  const int c = lc_class(olen[p], np);
  if (c < 0) return;
  int4* const t = c == 0 ? t0 : t1;
  const unsigned at = c == 0 ? c0[p] : c1[p];
  const unsigned chunk = (unsigned)kLcChunk[c], room = c == 0 ? room0 : room1;
  for (unsigned k = 0; k * chunk < np; ++k)
    if (at + k < room) t[at + k] = make_int4((int)p, (int)(first + k * chunk), (int)(np - k * chunk < chunk ? np - k * chunk : chunk), 0);
}

// ---- the enumeration ------------------------------------------------------------------------------------------------------
struct LcLists {
  const unsigned int *olen, *optr, *O, *P;
  unsigned long long* num;                               // [n] the numerators
  unsigned long long* tot;                               // [kLcTotals] triangles
};

template <int kThreads, int kSlots>
__global__ __launch_bounds__(kThreads) void lc_enum_kernel(LcLists a, const int4* __restrict__ tasks, const unsigned int* __restrict__ ntasks_p,
                                                           unsigned room) {
  constexpr int kWaves = kThreads / kWave;
  constexpr int kKeys = kSlots / 2;
  constexpr int kShift = 32 - (31 - __builtin_clz(kSlots));
  constexpr unsigned kMask = (unsigned)kSlots - 1u;
  __shared__ unsigned s_key[kSlots];
  __shared__ unsigned s_cnt[kSlots];
  __shared__ unsigned long long s_part[kWaves][2];
  __shared__ int s_next;
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const unsigned ntasks = *ntasks_p < room ? *ntasks_p : room;
  unsigned long long block_tri = 0;                      // (thread 0's)
  for (unsigned ti = blockIdx.x; ti < ntasks; ti += gridDim.x) {
    const int4 task = tasks[ti];
    const unsigned p = (unsigned)task.x, pf = (unsigned)task.y, np = (unsigned)task.z;
    const unsigned ob = a.optr[p], len = a.olen[p];
    unsigned credit_p = 0, tri = 0;
    // a streamed entry of partner q against the table: m_pq is q's bit + 1, acc the partner's credit
    auto look = [&](unsigned ent, unsigned m_pq, unsigned& acc) {
      const unsigned w = ent & kLcIdx;
      unsigned slot = (w * 0x9E3779B1u) >> kShift;
      unsigned t = s_key[slot];
      while (t != kLcEmpty && (t & kLcIdx) != w) { slot = (slot + 1u) & kMask; t = s_key[slot]; }
      if (t != kLcEmpty) {
        credit_p += 1u + (ent >> 31);
        acc += 1u + (t >> 31);
        ++tri;
        atomicAdd(&s_cnt[slot], m_pq);
      }
    };
    for (unsigned s0 = 0; s0 < len; s0 += kKeys) {       // the slices of the pivot's list
      const unsigned sl = len - s0 < (unsigned)kKeys ? len - s0 : (unsigned)kKeys;
      __syncthreads();                                   // the table is free: the flush before is done
      for (int i = tid; i < kSlots; i += kThreads) { s_key[i] = kLcEmpty; s_cnt[i] = 0u; }
      if (tid == 0) s_next = kWaves;
      __syncthreads();
      for (unsigned i = tid; i < sl; i += kThreads) {
        const unsigned ent = a.O[ob + s0 + i];
        unsigned slot = ((ent & kLcIdx) * 0x9E3779B1u) >> kShift;
        while (atomicCAS(&s_key[slot], kLcEmpty, ent) != kLcEmpty) slot = (slot + 1u) & kMask;   // (at most half full)
      }
      __syncthreads();
      const int nbatch = (int)((np + kWave - 1) / kWave);
      int b = kWaves > 1 ? wid : 0;
      while (b < nbatch) {                               // (b is the same in every lane of the wave)
        const unsigned qi = (unsigned)b * kWave + (unsigned)lane;
        const bool have = qi < np;
        const unsigned pent = have ? a.P[pf + qi] : kLcPad;
        const unsigned q = pent & kLcIdx, m_pq = 1u + (pent >> 31);
        const unsigned qb = have ? a.optr[q] : 0u, ql = have ? a.olen[q] : 0u;
        unsigned cq = 0;
        const bool by_lane = ql <= (unsigned)kLcLaneLen;
        if (have && by_lane) {
          for (unsigned k = 0; k < ql; k += 4) {
            const uint4 e4 = *reinterpret_cast<const uint4*>(a.O + qb + k);
            if (e4.x != kLcPad) look(e4.x, m_pq, cq);
            if (e4.y != kLcPad) look(e4.y, m_pq, cq);
            if (e4.z != kLcPad) look(e4.z, m_pq, cq);
            if (e4.w != kLcPad) look(e4.w, m_pq, cq);
          }
        }
        unsigned long long longs = __ballot(have && !by_lane);
        while (longs) {                                  // the longer partners, one after the other, by the whole wave
          const int l = __ffsll((long long)longs) - 1;
          longs &= longs - 1ull;
          const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)qb, l), ll = (unsigned)__builtin_amdgcn_readlane((int)ql, l);
          const unsigned lm = (unsigned)__builtin_amdgcn_readlane((int)m_pq, l);
          unsigned c = 0;
          for (unsigned k = 4u * (unsigned)lane; k < ll; k += 4u * kWave) {
            const uint4 e4 = *reinterpret_cast<const uint4*>(a.O + lb + k);
            if (e4.x != kLcPad) look(e4.x, lm, c);
            if (e4.y != kLcPad) look(e4.y, lm, c);
            if (e4.z != kLcPad) look(e4.z, lm, c);
            if (e4.w != kLcPad) look(e4.w, lm, c);
          }
          c = wave_sum_u32(c);
          if (lane == l) cq = c;
        }
        if (cq) {                                        // q's credit: beside its slot if it is in the table
          unsigned slot = (q * 0x9E3779B1u) >> kShift;
          unsigned t = s_key[slot];
          while (t != kLcEmpty && (t & kLcIdx) != q) { slot = (slot + 1u) & kMask; t = s_key[slot]; }
          if (t != kLcEmpty) atomicAdd(&s_cnt[slot], cq);
          else atomicAdd(&a.num[q], (unsigned long long)cq);
        }
        if (kWaves > 1) {
          if (lane == 0) b = atomicAdd(&s_next, 1);
          b = __builtin_amdgcn_readfirstlane(b);
        } else {
          ++b;
        }
      }
      __syncthreads();
      for (int i = tid; i < kSlots; i += kThreads) {
        const unsigned c = s_cnt[i];
        if (c) atomicAdd(&a.num[s_key[i] & kLcIdx], (unsigned long long)c);
      }
    }
    const unsigned long long wc = wave_sum_u64((unsigned long long)credit_p), wt = wave_sum_u64((unsigned long long)tri);
    __syncthreads();                                     // s_part is free
    if (lane == 0) { s_part[wid][0] = wc; s_part[wid][1] = wt; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long c = 0, t = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) { c += s_part[w][0]; t += s_part[w][1]; }
      if (c) atomicAdd(&a.num[p], c);
      block_tri += t;
    }
  }
  if (tid == 0 && block_tri) atomicAdd(&a.tot[blockIdx.x & (kLcTotals - 1)], block_tri);
}

// ---- the quotient and the record ------------------------------------------------------------------------------------------
// rec: [0] closed [1] wedges [2] the sum of d [3] max d [4] triangles ([5]: the symmetry check's flag, graph_common.hpp)
__global__ __launch_bounds__(kBlock) void lc_final_kernel(const unsigned int* __restrict__ sptr, const unsigned long long* __restrict__ num,
                                                          const unsigned long long* __restrict__ tot, Index n, float* __restrict__ out,
                                                          unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long s_sum[kWavesPerBlock][3];
  __shared__ unsigned s_max[kWavesPerBlock];
  unsigned long long closed = 0, wedges = 0, degs = 0;
  unsigned dmax = 0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    const unsigned d = sptr[v + 1] - sptr[v];
    const unsigned long long nm = num[v];
    float val = 0.f;
    if (d >= 2u) {
      val = (float)((double)nm / ((double)d * (double)(d - 1u)));
      wedges += (unsigned long long)d * (unsigned long long)(d - 1u);
    }
    out[v] = val;
    closed += nm;
    degs += d;
    dmax = d > dmax ? d : dmax;
  }
  closed = wave_sum_u64(closed);
  wedges = wave_sum_u64(wedges);
  degs = wave_sum_u64(degs);
  dmax = wave_max_u32(dmax);
  if (lane_id() == 0) { s_sum[wave_id()][0] = closed; s_sum[wave_id()][1] = wedges; s_sum[wave_id()][2] = degs; s_max[wave_id()] = dmax; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) t += s_sum[w][threadIdx.x];
    if (t) atomicAdd(&rec[threadIdx.x], t);
  } else if (threadIdx.x == 3) {
    unsigned m = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) m = s_max[w] > m ? s_max[w] : m;
    if (m) atomicMax(&rec[3], (unsigned long long)m);
  }
  if (blockIdx.x == 0 && wave_id() == 1) {               // (a whole wave: the sum is the wave's)
    const unsigned long long t = wave_sum_u64(tot[lane_id()]);
    if (lane_id() == 0) rec[4] = t;
  }
}

namespace {

grb_info lcc_zero(grb_vector lcc, grb_lcc_result* res) {
  GRB_TRY(ctx_init());
  GRB_TRY(grb_vector_set_storage(lcc, GRB_DENSE));
  if (lcc->nsize > 0) {
    GRB_HIP_TRY(hipMemsetAsync(lcc->d_val, 0, 4 * (size_t)lcc->nsize, ctx().stream));
    GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  }
  lcc->d_nnz = lcc->nsize;
  grb_lcc_result none = {};
  if (res) *res = none;
  return GRB_SUCCESS;
}

grb_info lcc_run(grb_vector lcc, grb_matrix A, bool directed, grb_lcc_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = A->nrows;
  const size_t nnz = (size_t)A->nvals;
  const size_t smax = directed ? 2 * nnz : nnz;          // S's entries at most; O's and P's are no more
  // (positions are 32-bit: O's with up to three fillings a list)
  if ((unsigned long long)smax + 4ull * (unsigned long long)n >= 0xfffffff0ull) return GRB_OUT_OF_MEMORY;
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the record, seven arrays of n + 1 words, the scan's totals, num, the values, S, O, P, the tasks
  const size_t vw = pad_words((size_t)n + 2), recw = pad_words(16 + 2 * kLcTotals);
  const size_t scanw = pad_words(device_scan_u32_scratch((long long)n + 1) / 4 + 1);
  const size_t sw = pad_words(smax + 4), ow = pad_words(smax + 4 * (size_t)n + 8);
  const size_t room0 = (size_t)n + smax / kLcChunk[0] + 2, room1 = (size_t)n + smax / kLcChunk[1] + 2;
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 4 * (recw + 7 * vw + scanw + 2 * vw + vw + sw + ow + sw + 4 * pad_words(room0) + 4 * pad_words(room1))));
  unsigned int* q = (unsigned int*)work.p;
  unsigned long long* d_rec = (unsigned long long*)q;                    // [0..7] the record, then kLcTotals partial counts
  unsigned long long* d_tot = d_rec + 8;
  q += recw;
  unsigned int* d_sptr = q; q += vw;
  unsigned int* d_olen = q; q += vw;
  unsigned int* d_optr = q; q += vw;
  unsigned int* d_pptr = q; q += vw;
  unsigned int* d_pcur = q; q += vw;
  unsigned int* d_c0 = q; q += vw;
  unsigned int* d_c1 = q; q += vw;
  unsigned int* d_scan = q; q += scanw;
  unsigned long long* d_num = (unsigned long long*)q; q += 2 * vw;
  float* d_out = (float*)q; q += vw;
  unsigned int* d_S = q; q += sw;
  unsigned int* d_O = q; q += ow;
  unsigned int* d_P = q; q += sw;
  int4* d_t0 = (int4*)q; q += 4 * pad_words(room0);
  int4* d_t1 = (int4*)q;
  GRB_TRY(dense_out_prepare(lcc, n));                    // before anything runs; lcc stays as it was until the end

  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(work.p, 0, 4 * (recw + 7 * vw + scanw + 2 * vw), s));   // the record, the counts, num
  const Index* rptr = A->csr.ptr;
  const Index* rind = A->csr.ind;
  const Index* cptr = directed ? A->csc.ptr : nullptr;
  const Index* cind = directed ? A->csc.ind : nullptr;
  if (!directed) launch_symmetry_check<false>(A, (unsigned int*)(d_rec + 5), s);
  const int wgrid = stream_grid(n, kWavesPerBlock), vgrid = (int)(((long long)n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(lc_merge_kernel<false>, dim3(wgrid), dim3(kBlock), 0, s, rptr, rind, cptr, cind, n, d_sptr, d_S);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_sptr, (long long)n + 1, d_scan));
  hipLaunchKernelGGL(lc_merge_kernel<true>, dim3(wgrid), dim3(kBlock), 0, s, rptr, rind, cptr, cind, n, d_sptr, d_S);
  hipLaunchKernelGGL(lc_olen_kernel, dim3(wgrid), dim3(kBlock), 0, s, (const unsigned int*)d_sptr, (const unsigned int*)d_S, n, d_olen, d_optr);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_optr, (long long)n + 1, d_scan));
  hipLaunchKernelGGL(lc_ofill_kernel, dim3(wgrid), dim3(kBlock), 0, s, (const unsigned int*)d_sptr, (const unsigned int*)d_S, n,
                     (const unsigned int*)d_olen, (const unsigned int*)d_optr, d_O, d_pptr);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_pptr, (long long)n + 1, d_scan));
  GRB_HIP_TRY(hipMemcpyAsync(d_pcur, d_pptr, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(lc_pfill_kernel, dim3(wgrid), dim3(kBlock), 0, s, n, (const unsigned int*)d_olen, (const unsigned int*)d_optr,
                     (const unsigned int*)d_O, (const unsigned int*)d_pptr, d_pcur, d_P);
  hipLaunchKernelGGL(lc_task_count_kernel, dim3(vgrid), dim3(kBlock), 0, s, (const unsigned int*)d_olen, (const unsigned int*)d_pptr, n, d_c0, d_c1);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_c0, (long long)n + 1, d_scan));
  GRB_TRY(device_exclusive_scan_u32_async(d_c1, (long long)n + 1, d_scan));
  hipLaunchKernelGGL(lc_task_fill_kernel, dim3(vgrid), dim3(kBlock), 0, s, (const unsigned int*)d_olen, (const unsigned int*)d_pptr, n,
                     (const unsigned int*)d_c0, (const unsigned int*)d_c1, d_t0, d_t1, (unsigned)room0, (unsigned)room1);
  // ---- the enumeration: the workgroups' tasks first (the long ones), then the waves'
  LcLists lists = {d_olen, d_optr, d_O, d_P, d_num, d_tot};
  const int grid1 = (int)(room1 < 16384 ? room1 : 16384), grid0 = (int)(room0 < 65536 ? room0 : 65536);
  hipLaunchKernelGGL((lc_enum_kernel<kBlock, kLcSlots>), dim3(grid1), dim3(kBlock), 0, s, lists, (const int4*)d_t1, (const unsigned int*)(d_c1 + n),
                     (unsigned)room1);
  hipLaunchKernelGGL((lc_enum_kernel<kWave, kLcWaveSlots>), dim3(grid0), dim3(kWave), 0, s, lists, (const int4*)d_t0, (const unsigned int*)(d_c0 + n),
                     (unsigned)room0);
  hipLaunchKernelGGL(lc_final_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, (const unsigned int*)d_sptr, (const unsigned long long*)d_num,
                     (const unsigned long long*)d_tot, n, d_out, d_rec);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  unsigned long long h_rec[8];
  GRB_HIP_TRY(hipMemcpyAsync(h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // the call's one read
  if ((unsigned int)h_rec[5] != 0u) return GRB_INVALID_VALUE;            // A's CSR and CSC differ: not symmetric
  GRB_TRY(dense_out_commit(lcc, d_out, n, s));
  grb_lcc_result out = {};
  out.closed = (int64_t)h_rec[0];
  out.wedges = (int64_t)h_rec[1];
  out.edges = (int64_t)(h_rec[2] / 2);
  out.max_degree = (int32_t)h_rec[3];
  out.triangles = (int64_t)h_rec[4];
  GRB_HIP_TRY(hipEventElapsedTime(&out.loop_ms, ev.a, ev.b));
  if (res) *res = out;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the local clustering coefficient: the contract is the comment in include/grb_hip.h
grb_info grb_lcc(grb_vector lcc, grb_matrix A, int directed, grb_descriptor desc, grb_lcc_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!lcc || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || lcc->nsize != n) return GRB_DIMENSION_MISMATCH;
  if (directed != 0 && directed != 1) return GRB_INVALID_VALUE;
  if (lcc->dtype != GRB_F32 || (A->dtype != GRB_F32 && A->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (!A->csr.ptr && n > 0) return GRB_INVALID_OBJECT;
  if (directed && (A->csc_alias || !A->csc.ptr) && n > 0) return GRB_INVALID_OBJECT;   // a product result: no CSC of its own
  if (n == 0 || A->nvals == 0) return lcc_zero(lcc, result);
  return lcc_run(lcc, A, directed != 0, result);
}
