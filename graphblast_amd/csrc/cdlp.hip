// cdlp.hip -- community detection by synchronous label propagation on the device: grb_cdlp.  The contract is the comment
// in include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definition is Graphalytics' and
// LAGraph's: L(v) <- the most frequent label among v's neighbours, the smallest one on a tie.
//
// The update is a per-row mode, no monoid.  What makes it one pass over a list: a label's count is kept in a table under
// integer atomic adds that RETURN the count before the add.  Every adder knows "after my add this label stood at c"; c is
// never above the label's final count and whoever adds last sees exactly that.  So the largest (c, then the smallest
// label) over all adds of a list IS the mode, and nobody reads the table back.
//   lists of up to kCdTinyLen entries   eight lanes a vertex, no table: a lane an entry, the counts by comparing all pairs
//   ... up to kCdWaveLen                a wave a vertex, the same
//   ... up to kCdSmallLen               a one-wave workgroup a vertex: indices streamed 16 bytes a lane, eight labels
//                                       gathered per lane and step, an LDS hash table of kCdSmallSlots (label, count) pairs
//   ... up to kCdBlockLen               the same with 256 threads and kCdSlots pairs
//   longer ones                         1024 threads a vertex and one of kCdPool .. kCdPoolMax count arrays of n words in
//                                       global memory (labels are < n): exact for any length and any number of distinct
//                                       labels.  The adds of the lanes that hold the same label as the wave's first lane go
//                                       out as one.  A second walk over the list puts the zeros back.
// In the directed case a vertex's list is its CSR row followed by its CSC column, walked into the same table.
// activity    an iteration evaluates only the vertices with a neighbour whose label the iteration before changed.  push: a
//             task that changed its vertex's label marks, with atomicOr into a bitmap, the vertices that have it as a
//             neighbour -- its CSC column (undirected) or both lists (directed) -- and one compaction kernel turns the
//             bitmap into the five work lists of the next iteration (and clears it).  A matrix without a CSC of its own
//             (undirected only) cannot push: there every vertex's task first looks whether any neighbour is in the bitmap
//             of changed vertices, and evaluates only then (pull).  grb_cdlp_set_skip(0): the full lists every time.
//             After an iteration that changed ALL n vertices the next one is due on the full lists whatever it marks, and
//             if it changes them all again so is the one after: it runs without marks (a grid, a path: every vertex
//             changes every time, and the marks would be a third of the time), and only if it then changes fewer than n
//             are the marks made after the fact, by one more kernel and one more host read.
// The host reads one record per iteration: {changed, the five list lengths, evaluated}.  Nothing is allocated in the loop.
#include "graph_common.hpp"

namespace grb {

constexpr int kCdTinyLen = 8;                            // a list of up to this many entries: eight lanes
constexpr int kCdWaveLen = 64;                           // ... a wave
constexpr int kCdSmallLen = 512;                         // ... a one-wave workgroup with a small LDS table
constexpr int kCdSmallSlots = 2 * kCdSmallLen;           // its (label, count) pairs: 8 KiB, at most half full
constexpr int kCdBlockLen = 2048;                        // ... a workgroup with the LDS table; a longer one: a global count array
constexpr int kCdSlots = 2 * kCdBlockLen;                // (label, count) pairs of the LDS table: 32 KiB, at most half full
constexpr int kCdLongThreads = 1024;                     // threads that walk a longer list
constexpr int kCdPool = 32;                              // global count arrays, i.e. long lists evaluated at once: at least this many,
constexpr int kCdPoolMax = 256;                          // ... at most this many (a workgroup each: the CUs),
constexpr size_t kCdPoolBytes = (size_t)128 << 20;       // ... and between the two as many as fit in this: the Infinity Cache
                                                         // holds it (RMAT-20 with 128 arrays, 512 MiB: 0.72 against 1.1 ms per
                                                         // full iteration in this kernel, and 30 ms to allocate them)
constexpr int kCdTile = 2048;                            // vertices one workgroup of the compaction takes: 64 bitmap words
constexpr int kCdClasses = 5;
constexpr unsigned kCdEmpty = 0xffffffffu;
static_assert(kCdWaveLen == kWave && kCdTile == 8 * kBlock && (kCdSlots & (kCdSlots - 1)) == 0 &&
              (kCdSmallSlots & (kCdSmallSlots - 1)) == 0, "sizes");

struct CdArgs {
  const Index *rptr, *rind;                              // the CSR: every vertex's first list
  const Index *cptr, *cind;                              // directed: the CSC, the second list; else nullptr
  const Index *mptr, *mind;                              // undirected push: the CSC, whom a changed vertex marks; else nullptr
  Index n;
  const int* lab_in;                                     // L_t
  int* lab_out;                                          // L_t+1, = L_t where nothing is written
  unsigned int* act;                                     // push: next iteration's activity bitmap (nullptr: no marks)
  const unsigned int* chg_prev;                          // pull: who changed in the iteration before (nullptr: evaluate all)
  unsigned int* chg_next;                                // pull: who changes in this one (nullptr: not kept)
  unsigned int* rec;                                     // [0] changed [1..5] next list lengths [6] evaluated (pull) [7] communities
};

template <int kSlots> __device__ __forceinline__ unsigned cd_hash(unsigned x) { return (x * 0x9E3779B1u) >> (32 - (31 - __builtin_clz(kSlots))); }
__device__ __forceinline__ bool cd_bit(const unsigned int* __restrict__ bits, Index v) { return (bits[v >> 5] >> (v & 31)) & 1u; }
__device__ __forceinline__ void cd_mark(unsigned int* __restrict__ bits, Index w) {
  const unsigned int b = 1u << (w & 31);
  if (!(bits[w >> 5] & b)) atomicOr(&bits[w >> 5], b);   // (a stale read costs one more atomic, nothing else)
}

// f(u) for every entry u of ind[b, e), thread t of nt: 16 bytes a lane where a whole aligned quad lies inside, eight
// entries per lane and step; g(u) turns an entry into what f takes (a gather: all eight are in flight before the first f).
// ind may be an adopted array that starts at any 4-byte boundary: then every quad goes entry by entry (the same for the
// whole launch, so no wave diverges on it)
template <typename G, typename F>
__device__ __forceinline__ void cd_stream(const Index* __restrict__ ind, Index b, Index e, int t, int nt, G g, F f) {
  const bool wide = (reinterpret_cast<uintptr_t>(ind) & 15u) == 0;
  for (Index x0 = (b & ~3) + 4 * t; x0 < e; x0 += 8 * nt) {
    Index u[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const Index x = x0 + h * 4 * nt;
      if (wide && x >= b && x + 4 <= e) {
        const int4 q = *reinterpret_cast<const int4*>(ind + x);
        u[4 * h] = q.x; u[4 * h + 1] = q.y; u[4 * h + 2] = q.z; u[4 * h + 3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) u[4 * h + k] = (x + k >= b && x + k < e) ? ind[x + k] : -1;
      }
    }
    int l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) l[k] = g(u[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (l[k] >= 0) f(l[k]);
  }
}

// the max / min of a value over aligned groups of G lanes, in every lane of the group (all 64 lanes active)
template <int G> __device__ __forceinline__ unsigned cd_group_max(unsigned v) {
  if constexpr (G == kWave) return wave_max_u32(v);
  else return group_reduce(v, G, [](unsigned a, unsigned b) { return a > b ? a : b; });
}
template <int G> __device__ __forceinline__ unsigned cd_group_min(unsigned v) {
  if constexpr (G == kWave) return wave_min_u32(v);
  else return group_reduce(v, G, [](unsigned a, unsigned b) { return a < b ? a : b; });
}

// ---- lists of up to G entries: G lanes a vertex -------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kBlock) void cd_group_kernel(CdArgs a, const Index* __restrict__ list, int count) {
  __shared__ unsigned int s_sum[2][kWavesPerBlock];
  constexpr int kGroups = kBlock / G;
  const int i = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const int gbase = lane_id() & ~(G - 1);                // the group's first lane in its wave
  unsigned int n_changed = 0, n_eval = 0;
  // (the bound is the same for every lane of a wave: its first group's task)
  for (long long t0 = (long long)blockIdx.x * kGroups; t0 + (wave_id() * (kWave / G)) < count; t0 += (long long)gridDim.x * kGroups) {
    const long long t = t0 + grp;
    const bool live = t < count;
    const Index v = live ? list[t] : 0;
    Index rb = 0, re = 0, cb = 0, ce = 0;
    if (live) {
      rb = a.rptr[v];
      re = a.rptr[v + 1];
      if (a.cptr) { cb = a.cptr[v]; ce = a.cptr[v + 1]; }
    }
    const int rlen = re - rb, len = rlen + (ce - cb);    // <= G
    Index u = -1;
    if (i < len) u = i < rlen ? a.rind[rb + i] : a.cind[cb + (i - rlen)];
    const bool valid = u != v && (unsigned)u < (unsigned)a.n;
    bool go = live;
    if (a.chg_prev) {                                    // pull: only where a neighbour changed
      const unsigned hit = valid && cd_bit(a.chg_prev, u) ? 1u : 0u;
      go = cd_group_max<G>(hit) != 0u;
    }
    const int l = valid && go ? a.lab_in[u] : -1;
    unsigned cnt = 0;
    if constexpr (G == kWave) {
      for (int k = 0; k < len; ++k) cnt += __builtin_amdgcn_readlane(l, k) == l ? 1u : 0u;
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k) cnt += __shfl(l, gbase + k, kWave) == l ? 1u : 0u;
    }
    if (l < 0) cnt = 0u;
    const unsigned best_cnt = cd_group_max<G>(cnt);
    const unsigned best = cd_group_min<G>(cnt == best_cnt && l >= 0 ? (unsigned)l : kCdEmpty);
    bool changed = false;
    if (go && best_cnt > 0u) {                           // (uniform over the group)
      changed = (int)best != a.lab_in[v];
      if (i == 0) {
        ++n_eval;
        if (changed) {
          a.lab_out[v] = (int)best;
          ++n_changed;
          if (a.chg_next) atomicOr(&a.chg_next[v >> 5], 1u << (v & 31));
        }
      }
    }
    if (changed && a.act) {
      if (a.cptr) {                                      // directed: both lists, the entries at hand
        if (valid) cd_mark(a.act, u);
      } else {
        const Index mb = a.mptr[v], me = a.mptr[v + 1];
        for (Index x = mb + i; x < me; x += G) {
          const Index w = a.mind[x];
          if (w != v && (unsigned)w < (unsigned)a.n) cd_mark(a.act, w);
        }
      }
    }
  }
  n_changed = wave_sum_u32(n_changed);
  n_eval = wave_sum_u32(n_eval);
  if (lane_id() == 0) { s_sum[0][wave_id()] = n_changed; s_sum[1][wave_id()] = n_eval; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned int tot = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) tot += s_sum[threadIdx.x][w];
    if (tot) atomicAdd(&a.rec[threadIdx.x == 0 ? 0 : 6], tot);
  }
}

// ---- longer lists: a workgroup of kThreads a vertex ---------------------------------------------------------------------
// kSlots > 0: an LDS table of that many pairs.  kSlots == 0: pool + blockIdx.x * n, a count array of this workgroup's own,
// all zero between tasks
template <int kThreads, int kSlots>
__global__ __launch_bounds__(kThreads) void cd_block_kernel(CdArgs a, const Index* __restrict__ list, int count, unsigned int* __restrict__ pool) {
  constexpr bool kLong = kSlots == 0;
  constexpr int kWaves = kThreads / kWave;
  __shared__ unsigned int s_key[kLong ? 1 : kSlots];
  __shared__ unsigned int s_cnt[kLong ? 1 : kSlots];
  __shared__ unsigned int s_c[kWaves], s_l[kWaves];
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  unsigned int* const table = kLong ? pool + (size_t)blockIdx.x * (size_t)a.n : nullptr;
  unsigned int n_changed = 0, n_eval = 0;                // (thread 0's)
  for (int t = blockIdx.x; t < count; t += gridDim.x) {
    const Index v = list[t];
    const Index rb = a.rptr[v], re = a.rptr[v + 1];
    const Index cb = a.cptr ? a.cptr[v] : 0, ce = a.cptr ? a.cptr[v + 1] : 0;
    auto both = [&](auto g, auto f) {
      cd_stream(a.rind, rb, re, tid, kThreads, g, f);
      if (a.cptr) cd_stream(a.cind, cb, ce, tid, kThreads, g, f);
    };
    if (a.chg_prev) {                                    // pull: only where a neighbour changed
      int hit = 0;
      both([&](Index u) { return u != v && (unsigned)u < (unsigned)a.n && cd_bit(a.chg_prev, u) ? 1 : -1; }, [&](int) { hit = 1; });
      if (!__syncthreads_or(hit)) continue;
    }
    if constexpr (!kLong) {
      for (int s = tid; s < kSlots; s += kThreads) { s_key[s] = kCdEmpty; s_cnt[s] = 0u; }
      __syncthreads();
    }
    unsigned bc = 0, bl = kCdEmpty;                      // this thread's best: the count a label stood at after an add of its own
    auto label = [&](Index u) { return u != v && (unsigned)u < (unsigned)a.n ? a.lab_in[u] : -1; };
    auto better = [&](unsigned c, unsigned l) {
      if (c > bc || (c == bc && l < bl)) { bc = c; bl = l; }
    };
    if constexpr (kLong) {
      both(label, [&](int l) {
        // the lanes here that hold the first one's label add together
        const int first = __builtin_amdgcn_readfirstlane(l);
        const unsigned long long same = __ballot(l == first);
        if (l != first) {
          better(atomicAdd(&table[l], 1u) + 1u, (unsigned)l);
        } else if (lane == __ffsll((long long)same) - 1) {
          const unsigned k = (unsigned)__popcll(same);
          better(atomicAdd(&table[l], k) + k, (unsigned)l);
        }
      });
    } else {
      both(label, [&](int l) {
        unsigned h = cd_hash<kLong ? 2 : kSlots>((unsigned)l);
        for (;;) {                                       // (at most half full: an empty slot comes)
          const unsigned was = atomicCAS(&s_key[h], kCdEmpty, (unsigned)l);
          if (was == kCdEmpty || was == (unsigned)l) break;
          h = (h + 1u) & (unsigned)(kSlots - 1);
        }
        better(atomicAdd(&s_cnt[h], 1u) + 1u, (unsigned)l);
      });
    }
    const unsigned wc = wave_max_u32(bc);
    const unsigned wl = wave_min_u32(bc == wc ? bl : kCdEmpty);
    if (lane == 0) { s_c[wid] = wc; s_l[wid] = wl; }
    __syncthreads();
    unsigned best_cnt = 0, best = kCdEmpty;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const unsigned c = s_c[w], l = s_l[w];
      if (c > best_cnt || (c == best_cnt && l < best)) { best_cnt = c; best = l; }
    }
    const bool changed = best_cnt > 0u && (int)best != a.lab_in[v];   // (uniform over the workgroup)
    if (tid == 0 && best_cnt > 0u) {
      ++n_eval;
      if (changed) {
        a.lab_out[v] = (int)best;
        ++n_changed;
        if (a.chg_next) atomicOr(&a.chg_next[v >> 5], 1u << (v & 31));
      }
    }
    if constexpr (kLong) {                               // the zeros back: every add above has returned
      both(label, [&](int l) { __hip_atomic_store(&table[l], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
      __threadfence();
    }
    if (changed && a.act) {
      auto whom = [&](Index w) { return w != v && (unsigned)w < (unsigned)a.n ? w : -1; };
      auto mark = [&](int w) { cd_mark(a.act, w); };
      if (a.cptr) both(whom, mark);
      else cd_stream(a.mind, a.mptr[v], a.mptr[v + 1], tid, kThreads, whom, mark);
    }
    __syncthreads();                                     // s_c / s_l and the table are free again
  }
  if (tid == 0) {
    if (n_changed) atomicAdd(&a.rec[0], n_changed);
    if (n_eval) atomicAdd(&a.rec[6], n_eval);
  }
}

// ---- the work lists -----------------------------------------------------------------------------------------------------
// kAll true: every vertex with a non-empty N(v) (a list of three or more entries holds an off-diagonal one: a row stores
// its diagonal once).  kAll false: the vertices marked in act, which is cleared.  lists[c * n ..]: class c; rec[1 + c]: its
// length (added to).  Order inside a list is whatever the workgroups' atomics make it; the update is synchronous.
template <bool kAll>
__global__ __launch_bounds__(kBlock) void cd_compact_kernel(CdArgs a, unsigned int* __restrict__ act, Index* __restrict__ lists) {
  __shared__ unsigned int s_cnt[kWavesPerBlock][kCdClasses];
  __shared__ unsigned int s_base[kCdClasses];
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const long long base = (long long)blockIdx.x * kCdTile;
  unsigned cls_bits = 0;                                 // 3 bits a step: class + 1, 0 = not listed
  unsigned wc[kCdClasses] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kCdTile / kBlock; ++k) {
    const long long v = base + k * kBlock + tid;
    int cls = -1;
    if (v < a.n && (kAll || cd_bit(act, (Index)v))) {
      const Index rb = a.rptr[v], re = a.rptr[v + 1];
      const Index cb = a.cptr ? a.cptr[v] : 0, ce = a.cptr ? a.cptr[v + 1] : 0;
      const int len = (re - rb) + (ce - cb);
      bool some = !kAll || len >= 3;
      if (kAll && !some) {
        for (Index x = rb; x < re; ++x) some |= a.rind[x] != (Index)v;
        for (Index x = cb; x < ce; ++x) some |= a.cind[x] != (Index)v;
      }
      if (some) cls = len <= kCdTinyLen ? 0 : len <= kCdWaveLen ? 1 : len <= kCdSmallLen ? 2 : len <= kCdBlockLen ? 3 : 4;
    }
    cls_bits |= (unsigned)(cls + 1) << (3 * k);
#pragma unroll
    for (int c = 0; c < kCdClasses; ++c) wc[c] += (unsigned)__popcll(__ballot(cls == c));
  }
  if (lane == 0)
    for (int c = 0; c < kCdClasses; ++c) s_cnt[wid][c] = wc[c];
  __syncthreads();
  if (tid < kCdClasses) {
    unsigned tot = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) tot += s_cnt[w][tid];
    s_base[tid] = tot ? atomicAdd(&a.rec[1 + tid], tot) : 0u;
  }
  if (!kAll && tid < kCdTile / 32 && base + 32 * tid < a.n) act[base / 32 + tid] = 0u;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int c = 0; c < kCdClasses; ++c) {
    unsigned at = s_base[c];
    for (int w = 0; w < wid; ++w) at += s_cnt[w][c];
#pragma unroll
    for (int k = 0; k < kCdTile / kBlock; ++k) {
      const bool mine = ((cls_bits >> (3 * k)) & 7u) == (unsigned)(c + 1);
      const unsigned long long m = __ballot(mine);
      if (mine) lists[(size_t)c * (size_t)a.n + at + (unsigned)__popcll(m & below)] = (Index)(base + k * kBlock + tid);
      at += (unsigned)__popcll(m);
    }
  }
}

// The marks after the fact, a wave a vertex: whoever's label the iteration changed marks whom it is a neighbour of (an
// iteration that ran without marks because the one before had changed every vertex, and then did not change them all)
__global__ __launch_bounds__(kBlock) void cd_marks_kernel(CdArgs a) {
  const int lane = lane_id();
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < a.n; v += (long long)gridDim.x * kWavesPerBlock) {
    if (a.lab_in[v] == a.lab_out[v]) continue;           // (the same for the whole wave)
    auto walk = [&](const Index* __restrict__ ptr, const Index* __restrict__ ind) {
      for (Index x = ptr[v] + lane; x < ptr[v + 1]; x += kWave) {
        const Index w = ind[x];
        if (w != (Index)v && (unsigned)w < (unsigned)a.n) cd_mark(a.act, w);
      }
    };
    if (a.cptr) { walk(a.rptr, a.rind); walk(a.cptr, a.cind); }
    else walk(a.mptr, a.mind);
  }
}

// ---- the labels in and out ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cd_iota_kernel(int* __restrict__ lab, Index n) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v < n) lab[v] = (int)v;
}
// a sparse init: lab (all -1 before) gets the stored values at their indices
__global__ __launch_bounds__(kBlock) void cd_scatter_kernel(const Index* __restrict__ ind, const int* __restrict__ val, Index nvals, Index n,
                                                            int* __restrict__ lab) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k < nvals && (unsigned)ind[k] < (unsigned)n) lab[ind[k]] = val[k];
}
// flag |= 1 when a label lies outside 0 .. n - 1
__global__ __launch_bounds__(kBlock) void cd_check_kernel(const int* __restrict__ lab, Index n, unsigned int* __restrict__ flag) {
  bool bad = false;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock)
    bad |= (unsigned)lab[v] >= (unsigned)n;
  if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(flag, 1u);
}
// seen[l] = 1 for every label l in use (seen: n words, all zero before; plain stores of the same value, no atomics: the
// vertices of one large community would queue up on its word)
__global__ __launch_bounds__(kBlock) void cd_seen_kernel(const int* __restrict__ lab, Index n, int* __restrict__ seen) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    const unsigned l = (unsigned)lab[v];
    if (l < (unsigned)n) seen[l] = 1;
  }
}
// rec[7] += the labels in use
__global__ __launch_bounds__(kBlock) void cd_communities_kernel(const int* __restrict__ seen, Index n, unsigned int* __restrict__ rec) {
  __shared__ unsigned int s_sum[kWavesPerBlock];
  unsigned int first = 0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) first += seen[v] != 0 ? 1u : 0u;
  first = wave_sum_u32(first);
  if (lane_id() == 0) s_sum[wave_id()] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int tot = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) tot += s_sum[w];
    if (tot) atomicAdd(&rec[7], tot);
  }
}

namespace {

int g_cd_skip = 1;

inline int cd_grid(long long items) { return (int)((items + kBlock - 1) / kBlock > 0 ? (items + kBlock - 1) / kBlock : 1); }
grb_info cdlp_run(grb_vector labels, grb_matrix A, grb_vector init, bool directed, int max_iter, grb_cdlp_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = A->nrows;
  const bool own_csc = !A->csc_alias && A->csc.ptr != nullptr;
  const bool pull = !directed && !own_csc;               // nobody to push to: every task looks at its neighbours first
  const bool skip = g_cd_skip != 0;
  grb_cdlp_result out = {};
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- two label arrays, two bitmaps, the five lists, the record: one allocation
  const size_t lw = pad_words((size_t)n), bw = pad_words(((size_t)n + 31) / 32 + 1);
  EwmBuf work, pool;
  GRB_TRY(ewm_alloc(&work, 4 * (2 * lw + 2 * bw + kCdClasses * lw + 64)));
  unsigned int* d_rec = (unsigned int*)work.p;           // [0..7] as CdArgs::rec, [8] a label out of range
  int* d_lab[2] = {(int*)(d_rec + 64), (int*)(d_rec + 64) + lw};
  unsigned int* d_bits[2] = {(unsigned int*)(d_lab[1] + lw), (unsigned int*)(d_lab[1] + lw) + bw};
  Index* d_lists = (Index*)(d_bits[1] + bw);
  GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 256, s));
  // ---- L_0
  if (!init) {
    hipLaunchKernelGGL(cd_iota_kernel, dim3(cd_grid(n)), dim3(kBlock), 0, s, d_lab[0], n);
  } else {
    if (init->vec_type == GRB_DENSE) {
      GRB_HIP_TRY(hipMemcpyAsync(d_lab[0], init->d_val, 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
    } else {
      GRB_HIP_TRY(hipMemsetAsync(d_lab[0], 0xff, 4 * (size_t)n, s));
      hipLaunchKernelGGL(cd_scatter_kernel, dim3(cd_grid(n)), dim3(kBlock), 0, s, init->s_ind, (const int*)init->s_val, n, n, d_lab[0]);
    }
    hipLaunchKernelGGL(cd_check_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_lab[0], n, d_rec + 8);
  }
  GRB_HIP_TRY(hipGetLastError());
  CdArgs a = {};
  a.rptr = A->csr.ptr;
  a.rind = A->csr.ind;
  if (directed) { a.cptr = A->csc.ptr; a.cind = A->csc.ind; }
  else if (!pull) { a.mptr = A->csc.ptr; a.mind = A->csc.ind; }
  a.n = n;
  a.rec = d_rec;
  // ---- the full lists
  GRB_HIP_TRY(hipMemsetAsync(d_bits[0], 0, 4 * 2 * bw, s));
  const int tiles = (int)(((long long)n + kCdTile - 1) / kCdTile);
  hipLaunchKernelGGL(cd_compact_kernel<true>, dim3(tiles), dim3(kBlock), 0, s, a, (unsigned int*)nullptr, d_lists);
  GRB_HIP_TRY(hipGetLastError());
  unsigned int h_rec[16];
  GRB_HIP_TRY(hipMemcpyAsync(h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  if (h_rec[8] != 0u) return GRB_INVALID_INDEX;
  unsigned int cnt[kCdClasses];
  for (int c = 0; c < kCdClasses; ++c) cnt[c] = h_rec[1 + c];   // together: the vertices with a non-empty N(v)
  size_t fit = kCdPoolBytes / (4 * (size_t)n);
  fit = fit < (size_t)kCdPool ? (size_t)kCdPool : fit > (size_t)kCdPoolMax ? (size_t)kCdPoolMax : fit;
  const int npool = cnt[4] < fit ? (int)cnt[4] : (int)fit;
  if (npool > 0) {
    GRB_TRY(ewm_alloc(&pool, 4 * (size_t)npool * (size_t)n));
    GRB_HIP_TRY(hipMemsetAsync(pool.p, 0, 4 * (size_t)npool * (size_t)n, s));
  }
  GRB_TRY(dense_out_prepare(labels, n));                 // labels is as it was until the result is there
  if (pull && skip) GRB_HIP_TRY(hipMemsetAsync(d_bits[0], 0xff, 4 * bw, s));   // iteration 1: everybody's neighbours "changed"
  // ---- the iterations
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  int cur = 0;
  bool all_changed = false;                              // the iteration before changed every vertex: this one runs without marks
  for (int it = 1; it <= max_iter; ++it) {
    const int nxt = cur ^ 1;
    GRB_HIP_TRY(hipMemcpyAsync(d_lab[nxt], d_lab[cur], 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 32, s));
    a.lab_in = d_lab[cur];
    a.lab_out = d_lab[nxt];
    const bool push = skip && !pull;
    a.act = push && !all_changed ? d_bits[0] : nullptr;
    a.chg_prev = skip && pull ? d_bits[cur] : nullptr;
    a.chg_next = skip && pull ? d_bits[nxt] : nullptr;
    if (a.chg_next) GRB_HIP_TRY(hipMemsetAsync(d_bits[nxt], 0, 4 * bw, s));
    const Index* lc[kCdClasses];
    for (int c = 0; c < kCdClasses; ++c) lc[c] = d_lists + (size_t)c * (size_t)n;
    auto groups = [](unsigned int tasks, int per_block) { const long long b = ((long long)tasks + per_block - 1) / per_block; return (int)(b < 8192 ? b : 8192); };
    if (cnt[0] > 0u)
      hipLaunchKernelGGL(cd_group_kernel<kCdTinyLen>, dim3(groups(cnt[0], kBlock / kCdTinyLen)), dim3(kBlock), 0, s, a, lc[0], (int)cnt[0]);
    if (cnt[1] > 0u)
      hipLaunchKernelGGL(cd_group_kernel<kCdWaveLen>, dim3(groups(cnt[1], kWavesPerBlock)), dim3(kBlock), 0, s, a, lc[1], (int)cnt[1]);
    if (cnt[2] > 0u)
      hipLaunchKernelGGL((cd_block_kernel<kWave, kCdSmallSlots>), dim3(groups(cnt[2], 1)), dim3(kWave), 0, s, a, lc[2], (int)cnt[2],
                         (unsigned int*)nullptr);
    if (cnt[3] > 0u)
      hipLaunchKernelGGL((cd_block_kernel<kBlock, kCdSlots>), dim3(groups(cnt[3], 1)), dim3(kBlock), 0, s, a, lc[3], (int)cnt[3],
                         (unsigned int*)nullptr);
    if (cnt[4] > 0u)
      hipLaunchKernelGGL((cd_block_kernel<kCdLongThreads, 0>), dim3(npool), dim3(kCdLongThreads), 0, s, a, lc[4], (int)cnt[4],
                         (unsigned int*)pool.p);
    if (a.act) hipLaunchKernelGGL(cd_compact_kernel<false>, dim3(tiles), dim3(kBlock), 0, s, a, a.act, d_lists);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(h_rec, d_rec, 32, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the iteration's one synchronisation
    out.iterations = it;
    out.changed = (int32_t)h_rec[0];
    out.evaluated += a.chg_prev ? (long long)h_rec[6] : (long long)cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4];
    cur = nxt;
    if (h_rec[0] == 0u) break;
    if (push && !a.act && h_rec[0] != (unsigned int)n && it < max_iter) {   // the marks after all, and the lists from them
      a.act = d_bits[0];
      hipLaunchKernelGGL(cd_marks_kernel, dim3(stream_grid(n, kWavesPerBlock)), dim3(kBlock), 0, s, a);
      hipLaunchKernelGGL(cd_compact_kernel<false>, dim3(tiles), dim3(kBlock), 0, s, a, a.act, d_lists);
      GRB_HIP_TRY(hipGetLastError());
      GRB_HIP_TRY(hipMemcpyAsync(h_rec, d_rec, 32, hipMemcpyDeviceToHost, s));
      GRB_HIP_TRY(hipStreamSynchronize(s));
    }
    if (a.act)
      for (int c = 0; c < kCdClasses; ++c) cnt[c] = h_rec[1 + c];
    all_changed = push && h_rec[0] == (unsigned int)n;   // (then the lists, marked or left alone, are the full ones)
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  // ---- the communities, and the labels out
  GRB_HIP_TRY(hipMemsetAsync(d_lab[cur ^ 1], 0, 4 * (size_t)n, s));   // (the other label array is free now)
  GRB_HIP_TRY(hipMemsetAsync(d_rec, 0, 32, s));
  hipLaunchKernelGGL(cd_seen_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_lab[cur], n, d_lab[cur ^ 1]);
  hipLaunchKernelGGL(cd_communities_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_lab[cur ^ 1], n, d_rec);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipMemcpyAsync(h_rec, d_rec, 32, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // every kernel has run: nothing can fail from here on
  GRB_TRY(dense_out_commit(labels, d_lab[cur], n, s));
  GRB_HIP_TRY(hipEventElapsedTime(&out.loop_ms, ev.a, ev.b));
  out.communities = (int32_t)h_rec[7];
  if (res) *res = out;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// community detection by label propagation: the contract is the comment in include/grb_hip.h
grb_info grb_cdlp(grb_vector labels, grb_matrix A, grb_vector init, int directed, int max_iter, grb_descriptor desc,
                  grb_cdlp_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!labels || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || labels->nsize != n || (init && init->nsize != n)) return GRB_DIMENSION_MISMATCH;
  if (max_iter < 1 || (directed != 0 && directed != 1)) return GRB_INVALID_VALUE;
  if (init) {
    const Index stored = init->vec_type == GRB_DENSE ? init->nsize : init->vec_type == GRB_SPARSE ? init->s_nvals : 0;
    if (stored != n) return GRB_INVALID_VALUE;
  }
  if (labels->dtype != GRB_I32 || (init && init->dtype != GRB_I32) || (A->dtype != GRB_F32 && A->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (!A->csr.ptr && n > 0) return GRB_INVALID_OBJECT;
  if (directed && (A->csc_alias || !A->csc.ptr) && n > 0) return GRB_INVALID_OBJECT;   // a product result: no CSC of its own
  if (n == 0) {
    GRB_TRY(grb_vector_set_storage(labels, GRB_DENSE));
    grb_cdlp_result none = {};
    none.iterations = 1;
    if (result) *result = none;
    return GRB_SUCCESS;
  }
  return cdlp_run(labels, A, init, directed != 0, max_iter, result);
}

// 1: an iteration evaluates only the vertices with a neighbour that changed (default); 0: all of them, every time
int grb_cdlp_set_skip(int on) { GRB_API_ENTER_HOST();
  const int was = g_cd_skip;
  if (on >= 0) g_cd_skip = on ? 1 : 0;
  return was;
}
