// ktruss.hip -- k-truss and edge trussness on the device: grb_ktruss, grb_trussness.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definitions are LAGraph's.
//
// The working graph lives on the device for the whole call, structure only (no value array of A is ever read):
//   ptr / ind   the survivors, both directions of every edge, columns ascending in every row
//   twin[e]     the position of (j, i) for entry e = (i, j); so the row of entry e is ind[twin[e]]
//   sup[e]      the triangles of the working graph that edge e lies in
//   orig[e]     the entry's position in G's arrays (G: A without its diagonal)
// prepare   the diagonal's place in every row by a search, a scan of the diagonal counts, a wave per row that copies the
//           row without it and finds every entry's twin by a search in the twin row (of A: the rows of G are still being
//           written).
// support   every undirected edge is intersected ONCE: by the endpoint whose current list is longer (ties: the lower id),
//           the owner.  The owner's list goes into LDS -- a bitmap over its column window where that is at most kKtBits
//           wide, a hash table of twice its length otherwise; a list longer than kKtHashLen that is no bitmap is taken in
//           slices of kKtHashLen entries, one table after the other, the counts adding up in registers -- and the
//           partner's list, the shorter one, is streamed past it 16 bytes per lane per step: a lane walks a partner of up
//           to kKtLaneLen entries, the wave together a longer one.  The count goes to sup[e] and sup[twin[e]]: one
//           writer per entry, no atomics on global memory.  A row of up to kKtWaveLen entries is one wave's task; a longer
//           row is cut into workgroup tasks of kKtTask partners each, every one of which builds the table again (a hub of
//           10^5 neighbours is 391 tasks).
// filter    select.hip's compaction over the flat entry list with the predicate sup >= k - 2: a count per 2048-entry tile,
//           a scan, a write pass that also makes the new pointers; the survivors' ind, sup, orig and (old) twin move, the
//           new position of every survivor is noted, and a second pass sends the twins through those positions.  Under
//           grb_trussness the entries that leave at level k get k - 1 at orig[e] of the output.
// tasks     the next support computation's task lists from the new pointers: counts, one scan, fill.
// One round is filter + tasks (+ the support computation on what is left); the host reads {survivors, wave tasks,
// workgroup tasks} once per round, the round's only synchronisation.  Nothing is allocated inside the loop: three sets of
// arrays (G's own, never overwritten, and two that alternate) are carved from one allocation up front.
#include "graph_common.hpp"

namespace grb {

constexpr int kKtWaveLen = 64;                           // a row of up to this many entries is one wave's task
constexpr int kKtLaneLen = 32;                           // a partner of up to this many entries is walked by one lane
constexpr int kKtBits = 4096;                            // a column window of up to this many columns is a bitmap
constexpr int kKtHashLen = 4096;                         // the most entries one hash table takes (a longer list: slices)
constexpr int kKtTask = 256;                             // partners of one workgroup task
constexpr int kKtWaveSlots = 2 * kKtWaveLen;             // hash slots of a wave task (and kKtBits / 32 bitmap words)
constexpr int kKtBlockSlots = 2 * kKtHashLen;            // hash slots of a workgroup task: 32 KiB of LDS
constexpr int kKtSteps = 8;                              // the filter: entries per lane,
constexpr int kKtWaveTile = kWave * kKtSteps;            // consecutive entries of one wave,
constexpr int kKtTile = kKtWaveTile * kWavesPerBlock;    // ... of one workgroup (select.hip's 2048)
constexpr unsigned kKtEmpty = 0xffffffffu;
static_assert(kKtBits / 32 <= kKtWaveSlots && kKtTask == kBlock && kKtWaveLen == kWave, "table sizes");

__device__ __forceinline__ unsigned kt_hash(unsigned x, int slots) { return (x * 0x9E3779B1u) >> (32 - (31 - __builtin_clz(slots))); }

// ---- prepare ------------------------------------------------------------------------------------------------------------
// where the diagonal lies in row r: dlo[r] its first position, cnt[r] how many entries hold it (0 or 1; cnt[n] = 0)
__global__ __launch_bounds__(kBlock) void kt_diag_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index n,
                                                         Index* __restrict__ dlo, unsigned int* __restrict__ cnt) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  if (r == n) { cnt[n] = 0u; return; }
  const Index a = index_lower_bound(ind, ptr[r], ptr[r + 1], (Index)r);
  const Index b = index_lower_bound(ind, a, ptr[r + 1], (Index)r + 1);
  dlo[r] = a;
  cnt[r] = (unsigned int)(b - a);
}

// A's position x of row r -> G's (the diagonal entries before it do not count)
__device__ __forceinline__ Index kt_g_pos(Index x, Index r, const Index* __restrict__ dlo, const unsigned int* __restrict__ off) {
  const Index nd = (Index)(off[r + 1] - off[r]);
  return x - (Index)off[r] - (x >= dlo[r] + nd ? nd : 0);
}

// a wave per row: G's pointers, the row without its diagonal, every entry's twin and orig (its own position)
__global__ __launch_bounds__(kBlock) void kt_prepare_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index n,
                                                            const Index* __restrict__ dlo, const unsigned int* __restrict__ off,
                                                            Index* __restrict__ g_ptr, Index* __restrict__ g_ind, Index* __restrict__ g_twin,
                                                            Index* __restrict__ g_orig, unsigned int* __restrict__ flag) {
  const int lane = lane_id();
  for (long long r = (long long)blockIdx.x * kWavesPerBlock + wave_id(); r < n; r += (long long)gridDim.x * kWavesPerBlock) {
    const Index pb = ptr[r], pe = ptr[r + 1];
    if (lane == 0) {
      g_ptr[r] = pb - (Index)off[r];
      if (r == n - 1) g_ptr[n] = pe - (Index)off[n];
    }
    for (Index x = pb + lane; x < pe; x += kWave) {
      const Index j = ind[x];
      if (j == (Index)r) continue;
      const Index y = kt_g_pos(x, (Index)r, dlo, off);
      // (j, r) is in row j: the structure is symmetric.  Where it is not (a caller of the CSR-only format vouched for it),
      // the entry becomes its own twin, nothing is read out of bounds, and the call fails on the flag
      Index t = -1;
      if (j >= 0 && j < n) {
        t = index_lower_bound(ind, ptr[j], ptr[j + 1], (Index)r);
        if (t >= ptr[j + 1] || ind[t] != (Index)r) t = -1;
      }
      if (t < 0) atomicOr(flag, 1u);
      g_ind[y] = t < 0 ? (Index)r : j;
      g_twin[y] = t < 0 ? y : kt_g_pos(t, j, dlo, off);
      g_orig[y] = y;
    }
  }
}

// ---- support ------------------------------------------------------------------------------------------------------------
// One task: the partners at entries [e0, e1) of the owner's row, at most kThreads of them, a thread each.
template <int kThreads, int kSlots>
__global__ __launch_bounds__(kThreads) void kt_support_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind,
                                                              const Index* __restrict__ twin, int* __restrict__ sup,
                                                              const int2* __restrict__ tasks) {
  __shared__ unsigned int tab[kSlots];
  const int tid = threadIdx.x, lane = lane_id();
  const int2 task = tasks[blockIdx.x];
  const Index e0 = task.x, e1 = task.y;
  const Index p = ind[twin[e0]];                         // the owner: the row of these entries
  const Index pb = ptr[p], pe = ptr[p + 1];
  const int plen = pe - pb;
  const bool whole = ind[pe - 1] - ind[pb] < kKtBits || plen <= kSlots / 2;   // one table holds the whole list
  const int nslices = whole ? 1 : (plen + kKtHashLen - 1) / kKtHashLen;
  // this thread's partner
  const Index e = e0 + tid;
  Index qb = 0, qe = 0;
  bool mine = false;
  if (e < e1) {
    const Index q = ind[e];
    qb = ptr[q];
    qe = ptr[q + 1];
    const int qlen = qe - qb;
    mine = plen > qlen || (plen == qlen && p < q);       // the longer list owns the edge, the lower id on a tie
  }
  const bool walk = mine && qe - qb <= kKtLaneLen;       // a lane walks a short partner
  unsigned long long together = __ballot(mine && !walk); // ... the wave streams a long one
  int acc = 0;
  for (int s = 0; s < nslices; ++s) {
    const Index t0 = whole ? pb : pb + s * kKtHashLen;
    const Index t1 = whole ? pe : (t0 + kKtHashLen < pe ? t0 + kKtHashLen : pe);
    const Index lo = ind[t0], hi = ind[t1 - 1];
    const bool bitmap = hi - lo < kKtBits;               // (uniform over the workgroup)
    __syncthreads();                                     // the lookups in the table before this one are over
    if (bitmap) {
      for (int i = tid; i < kKtBits / 32; i += kThreads) tab[i] = 0u;
      __syncthreads();
      for (Index x = t0 + tid; x < t1; x += kThreads) {
        const unsigned int d = (unsigned int)(ind[x] - lo);
        atomicOr(&tab[d >> 5], 1u << (d & 31u));
      }
    } else {
      for (int i = tid; i < kSlots; i += kThreads) tab[i] = kKtEmpty;
      __syncthreads();
      for (Index x = t0 + tid; x < t1; x += kThreads) {
        const unsigned int c = (unsigned int)ind[x];
        unsigned int h = kt_hash(c, kSlots);
        while (atomicCAS(&tab[h], kKtEmpty, c) != kKtEmpty) h = (h + 1u) & (unsigned int)(kSlots - 1);   // (at most half full)
      }
    }
    __syncthreads();
    auto hit = [&](Index c) -> int {
      if (c < lo || c > hi) return 0;
      if (bitmap) {
        const unsigned int d = (unsigned int)(c - lo);
        return (int)((tab[d >> 5] >> (d & 31u)) & 1u);
      }
      unsigned int h = kt_hash((unsigned int)c, kSlots);
      for (;;) {
        const unsigned int v = tab[h];
        if (v == (unsigned int)c) return 1;
        if (v == kKtEmpty) return 0;
        h = (h + 1u) & (unsigned int)(kSlots - 1);
      }
    };
    // entries [b, en) of a list, four at a time from position x (a multiple of four: 16 bytes, aligned; the arrays are
    // padded to a multiple of four entries, and what lies outside [b, en) is not looked at)
    auto four = [&](Index x, Index b, Index en) -> int {
      const int4 v = *reinterpret_cast<const int4*>(ind + x);
      int c = 0;
      if (x >= b && x < en) c += hit(v.x);
      if (x + 1 >= b && x + 1 < en) c += hit(v.y);
      if (x + 2 >= b && x + 2 < en) c += hit(v.z);
      if (x + 3 >= b && x + 3 < en) c += hit(v.w);
      return c;
    };
    if (walk)
      for (Index x = qb & ~3; x < qe; x += 4) acc += four(x, qb, qe);
    for (unsigned long long m = together; m != 0ull; m &= m - 1ull) {
      const int l = __ffsll((long long)m) - 1;
      const Index b = __builtin_amdgcn_readlane(qb, l), en = __builtin_amdgcn_readlane(qe, l);
      int c = 0;
      for (Index x = (b & ~3) + 4 * lane; x < en; x += 4 * kWave) c += four(x, b, en);
      c = (int)wave_sum_u32((unsigned int)c);
      if (lane == l) acc += c;
    }
  }
  if (mine) {
    sup[e] = acc;
    sup[twin[e]] = acc;
  }
}

// ---- filter -------------------------------------------------------------------------------------------------------------
// the largest r with ptr[r] <= x, for 0 <= x < ptr[nrows]: the row of entry x (select.hip's search: 64 probes a round)
__device__ inline Index kt_find_row(const Index* __restrict__ ptr, Index nrows, long long x, int lane) {
  long long lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const long long step = (hi - lo + kWave - 1) / kWave;
    const long long q = lo + (lane + 1) * step;
    const bool le = q < hi && (long long)ptr[q] <= x;
    lo += __popcll(__ballot(le)) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return (Index)lo;
}

struct KtSet {                                           // one working graph
  Index *ptr, *ind, *twin, *orig;
  int* sup;
};

// kWrite false: tiles[t] = the entries of tile t with sup >= thr.  kWrite true: tiles[t] is tile t's offset; the
// survivors move to `out` in their order (twin still the OLD position), pos[e] = where entry e went, the new pointers
// are written, and with truss != nullptr an entry that leaves gets `level` at orig[e] of truss.  info[0] = the survivors.
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void kt_filter_kernel(KtSet in, Index nrows, long long nnz, int thr, unsigned int* __restrict__ tiles,
                                                           int ntiles, KtSet out, Index* __restrict__ pos, int* __restrict__ truss,
                                                           int level, unsigned int* __restrict__ info) {
  __shared__ int s_wave[kWavesPerBlock];
  const int lane = lane_id(), wid = wave_id();
  const long long w0 = (long long)blockIdx.x * kKtTile + (long long)wid * kKtWaveTile;
  const long long w1 = w0 + kKtWaveTile < nnz ? w0 + kKtWaveTile : nnz;   // the wave's entries: [w0, w1)
  const bool live = w0 < nnz;                            // wave-uniform
  unsigned long long m[kKtSteps];
  int kept = 0;
#pragma unroll
  for (int k = 0; k < kKtSteps; ++k) {
    const long long e = w0 + k * kWave + lane;
    m[k] = __ballot(e < w1 && in.sup[e] >= thr);
    kept += __popcll(m[k]);
  }
  if (lane == 0) s_wave[wid] = kept;
  __syncthreads();
  if constexpr (!kWrite) {
    if (threadIdx.x == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) sum += s_wave[w];
      tiles[blockIdx.x] = (unsigned int)sum;
    }
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = tiles[ntiles];
    if (!live) return;
    unsigned int base = tiles[blockIdx.x];               // the wave's first place in the result
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) base += w < wid ? (unsigned int)s_wave[w] : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned int at = base;
#pragma unroll
    for (int k = 0; k < kKtSteps; ++k) {
      const long long e = w0 + k * kWave + lane;
      if ((m[k] >> lane) & 1ull) {
        const unsigned int to = at + (unsigned int)__popcll(m[k] & below);
        out.ind[to] = in.ind[e];
        out.twin[to] = in.twin[e];
        out.sup[to] = in.sup[e];
        out.orig[to] = in.orig[e];
        pos[e] = (Index)to;
      } else if (truss != nullptr && e < w1) {
        truss[in.orig[e]] = level;
      }
      at += (unsigned int)__popcll(m[k]);
    }
    // the new pointers of the rows whose old one lies in (w0, w1]: base + the survivors of the wave before it.  Those
    // that are 0 (the rows up to the row of entry 0) fall to the first wave.
    const Index rw = kt_find_row(in.ptr, nrows, w0, lane);
    if (w0 == 0)
      for (long long r = lane; r <= (long long)rw; r += kWave) out.ptr[r] = 0;
    for (long long r = (long long)rw + 1 + lane;; r += kWave) {
      bool ok = false;
      if (r <= nrows) {
        const Index p = in.ptr[r];
        ok = p <= w1;
        if (ok) {
          const int d = (int)(p - w0);                   // in (0, kKtWaveTile]
          int rank = 0;
#pragma unroll
          for (int k = 0; k < kKtSteps; ++k) {
            const int b = d - k * kWave;                 // the flags of step k below the old pointer
            const unsigned long long sel = b >= kWave ? ~0ull : b <= 0 ? 0ull : (1ull << b) - 1ull;
            rank += __popcll(m[k] & sel);
          }
          out.ptr[r] = (Index)(base + (unsigned int)rank);
        }
      }
      if (__ballot(ok) != ~0ull) break;
    }
  }
}

// the survivors' twins through the new positions (*count: the survivors)
__global__ __launch_bounds__(kBlock) void kt_retwin_kernel(Index* __restrict__ twin, const Index* __restrict__ pos,
                                                           const unsigned int* __restrict__ count) {
  const long long x = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (x < (long long)*count) twin[x] = pos[twin[x]];
}

// ---- tasks --------------------------------------------------------------------------------------------------------------
// cnt[r] = the wave tasks of row r (0 or 1), cnt[n + r] = its workgroup tasks, cnt[2 n] = 0: one scan serves both lists.  A
// row of one entry has no triangle.
__global__ __launch_bounds__(kBlock) void kt_task_count_kernel(const Index* __restrict__ ptr, Index n, unsigned int* __restrict__ cnt) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  if (r == n) { cnt[2 * (size_t)n] = 0u; return; }
  const int len = ptr[r + 1] - ptr[r];
  cnt[r] = len >= 2 && len <= kKtWaveLen ? 1u : 0u;
  cnt[(size_t)n + r] = len > kKtWaveLen ? (unsigned int)((len + kKtTask - 1) / kKtTask) : 0u;
}
// info[1] = the wave tasks, info[2] = the workgroup tasks
__global__ __launch_bounds__(kBlock) void kt_task_fill_kernel(const Index* __restrict__ ptr, Index n, const unsigned int* __restrict__ off,
                                                              int2* __restrict__ wave_tasks, int2* __restrict__ block_tasks,
                                                              unsigned int* __restrict__ info) {
  const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (r == 0) {
    info[1] = off[n];
    info[2] = off[2 * (size_t)n] - off[n];
  }
  if (r >= n) return;
  const Index pb = ptr[r], pe = ptr[r + 1];
  const int len = pe - pb;
  if (len < 2) return;
  if (len <= kKtWaveLen) {
    wave_tasks[off[r]] = make_int2(pb, pe);
    return;
  }
  unsigned int at = off[(size_t)n + r] - off[n];
  for (Index a = pb; a < pe; a += kKtTask) block_tasks[at++] = make_int2(a, a + kKtTask < pe ? a + kKtTask : pe);
}

// ---- output -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kt_values_kernel(const int* __restrict__ v, long long n, int f32, unsigned int* __restrict__ out) {
  const long long x = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (x >= n) return;
  if (f32) {
    const float f = (float)v[x];
    memcpy(&out[x], &f, 4);
  } else {
    out[x] = (unsigned int)v[x];
  }
}

namespace {

inline int kt_grid(long long items) { return (int)((items + kBlock - 1) / kBlock > 0 ? (items + kBlock - 1) / kBlock : 1); }
// C = the k-truss of A's graph with its supports (trussness false), or G with every edge's trussness (true)
grb_info truss_run(grb_matrix C, grb_matrix A, int k_in, bool trussness, grb_truss_result* res) {
  hipStream_t s = ctx().stream;
  const Index n = A->nrows;
  const long long nnz = A->csr.nvals;
  grb_truss_result out = {};
  out.kmax = trussness ? 2 : k_in;
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- prepare: the symmetry check and the diagonal, one read
  EwmBuf pre;
  const size_t scan_words = device_scan_u32_scratch(2 * (long long)n + 1) / 4 + 1;
  GRB_TRY(ewm_alloc(&pre, 4 * (pad_words((size_t)n + 1) * 2 + pad_words(scan_words) + 64)));
  unsigned int* d_info = (unsigned int*)pre.p;           // [0] survivors [1] wave tasks [2] workgroup tasks [3] asymmetric
  Index* d_dlo = (Index*)(d_info + 64);
  unsigned int* d_off = (unsigned int*)(d_dlo + pad_words((size_t)n + 1));
  unsigned int* d_scan = d_off + pad_words((size_t)n + 1);
  GRB_HIP_TRY(hipMemsetAsync(d_info, 0, 256, s));
  launch_symmetry_check<false>(A, d_info + 3, s);
  hipLaunchKernelGGL(kt_diag_kernel, dim3(kt_grid((long long)n + 1)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, n, d_dlo, d_off);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_off, (long long)n + 1, d_scan));
  unsigned int h_info[4] = {0, 0, 0, 0};
  unsigned int ndiag = 0;
  GRB_HIP_TRY(hipMemcpyAsync(&ndiag, d_off + n, 4, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipMemcpyAsync(h_info, d_info, 16, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  if (h_info[3] != 0u) return GRB_INVALID_VALUE;         // A's CSR and CSC differ: not symmetric
  const long long E0 = nnz - (long long)ndiag;
  out.edges = E0 / 2;
  // ---- the three sets, the positions, the trussness and the task lists: one allocation
  const size_t ew = pad_words((size_t)E0 + 4), pw = pad_words((size_t)n + 1);
  const size_t max_wave_tasks = (size_t)n, max_block_tasks = (size_t)(E0 / kKtTask + E0 / (kKtWaveLen + 1) + 1);
  const int max_tiles = (int)((E0 + kKtTile - 1) / kKtTile);
  const size_t tile_words = pad_words((size_t)max_tiles + 1 + device_scan_u32_scratch((long long)max_tiles + 1) / 4 + 1);
  const size_t cnt_words = pad_words(2 * (size_t)n + 1);
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 4 * (3 * (pw + 4 * ew) + 2 * ew + tile_words + cnt_words + 2 * pad_words(max_wave_tasks + 1) +
                                2 * pad_words(max_block_tasks + 1))));
  KtSet set[3];
  Index* q = (Index*)work.p;
  for (int i = 0; i < 3; ++i) {
    set[i].ptr = q; q += pw;
    set[i].ind = q; q += ew;
    set[i].twin = q; q += ew;
    set[i].orig = q; q += ew;
    set[i].sup = (int*)q; q += ew;
  }
  Index* d_pos = q; q += ew;
  int* d_truss = (int*)q; q += ew;
  unsigned int* d_tiles = (unsigned int*)q; q += tile_words;
  unsigned int* d_cnt = (unsigned int*)q; q += cnt_words;
  int2* d_wave_tasks = (int2*)q; q += 2 * pad_words(max_wave_tasks + 1);
  int2* d_block_tasks = (int2*)q;
  auto build_tasks = [&](const KtSet& g) -> grb_info {
    hipLaunchKernelGGL(kt_task_count_kernel, dim3(kt_grid((long long)n + 1)), dim3(kBlock), 0, s, g.ptr, n, d_cnt);
    GRB_TRY(device_exclusive_scan_u32_async(d_cnt, 2 * (long long)n + 1, d_scan));
    hipLaunchKernelGGL(kt_task_fill_kernel, dim3(kt_grid((long long)n + 1)), dim3(kBlock), 0, s, g.ptr, n, d_cnt, d_wave_tasks,
                       d_block_tasks, d_info);
    GRB_HIP_TRY(hipGetLastError());
    return GRB_SUCCESS;
  };
  long long E = E0;
  int cur = 0;
  if (E0 > 0) {
    hipLaunchKernelGGL(kt_prepare_kernel, dim3(stream_grid(n, kWavesPerBlock)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, n, d_dlo, d_off,
                       set[0].ptr, set[0].ind, set[0].twin, set[0].orig, d_info + 3);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(build_tasks(set[0]));
    GRB_HIP_TRY(hipMemcpyAsync(h_info, d_info, 16, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
    if (h_info[3] != 0u) return GRB_INVALID_VALUE;       // an entry without its twin
  }
  // ---- the rounds
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  int k = trussness ? 3 : k_in;
  bool need_support = true;
  while (E > 0) {
    const KtSet& g = set[cur];
    const int nxt = cur == 1 ? 2 : 1;
    if (need_support) {
      GRB_HIP_TRY(hipMemsetAsync(g.sup, 0, 4 * (size_t)E, s));
      if (h_info[1] > 0u)
        hipLaunchKernelGGL((kt_support_kernel<kWave, kKtWaveSlots>), dim3(h_info[1]), dim3(kWave), 0, s, g.ptr, g.ind, g.twin, g.sup,
                           d_wave_tasks);
      if (h_info[2] > 0u)
        hipLaunchKernelGGL((kt_support_kernel<kBlock, kKtBlockSlots>), dim3(h_info[2]), dim3(kBlock), 0, s, g.ptr, g.ind, g.twin, g.sup,
                           d_block_tasks);
      GRB_HIP_TRY(hipGetLastError());
      ++out.supports;
    }
    const int ntiles = (int)((E + kKtTile - 1) / kKtTile);
    GRB_HIP_TRY(hipMemsetAsync(d_tiles + ntiles, 0, 4, s));
    hipLaunchKernelGGL(kt_filter_kernel<false>, dim3(ntiles), dim3(kBlock), 0, s, g, n, E, k - 2, d_tiles, ntiles, set[nxt], d_pos,
                       (int*)nullptr, 0, d_info);
    GRB_TRY(device_exclusive_scan_u32_async(d_tiles, (long long)ntiles + 1, d_tiles + ntiles + 1));
    hipLaunchKernelGGL(kt_filter_kernel<true>, dim3(ntiles), dim3(kBlock), 0, s, g, n, E, k - 2, d_tiles, ntiles, set[nxt], d_pos,
                       trussness ? d_truss : (int*)nullptr, k - 1, d_info);
    hipLaunchKernelGGL(kt_retwin_kernel, dim3(kt_grid(E)), dim3(kBlock), 0, s, set[nxt].twin, d_pos, d_info);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(build_tasks(set[nxt]));
    GRB_HIP_TRY(hipMemcpyAsync(h_info, d_info, 16, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the round's one synchronisation
    ++out.rounds;
    const long long kept = (long long)h_info[0];
    const bool removed = kept < E;
    cur = nxt;
    E = kept;
    if (trussness) {
      if (removed) out.kmax = k - 1;                     // what leaves at level k was in the (k - 1)-truss
      else ++k;                                          // this level is done; the supports are still those of the graph
      need_support = removed;
    } else {
      if (!removed) break;
      need_support = true;
    }
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  // ---- the result: the survivors with their supports, or G with the trussness
  const KtSet& g = trussness ? set[0] : set[cur];
  const long long En = trussness ? E0 : E;
  const bool both = C->format != 1;
  Side r, c;
  auto side = [&](Side* sd) -> grb_info {
    GRB_TRY(ewm_alloc(&sd->ptr, 4 * ((size_t)n + 1)));
    GRB_TRY(ewm_alloc(&sd->ind, 4 * (size_t)(En > 0 ? En : 1)));
    GRB_TRY(ewm_alloc(&sd->val, 4 * (size_t)(En > 0 ? En : 1)));
    sd->nnz = (Index)En;
    sd->h_ptr.assign((size_t)n + 1, 0);
    return GRB_SUCCESS;
  };
  GRB_TRY(side(&r));
  if (both) GRB_TRY(side(&c));
  if (En > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(r.ptr.p, g.ptr, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemcpyAsync(r.ind.p, g.ind, 4 * (size_t)En, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(kt_values_kernel, dim3(kt_grid(En)), dim3(kBlock), 0, s, trussness ? d_truss : g.sup, En,
                       C->dtype == GRB_F32 ? 1 : 0, (unsigned int*)r.val.p);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(r.h_ptr.data(), g.ptr, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    if (both) {                                          // the structure is symmetric and so are the values: the CSC is a copy
      GRB_HIP_TRY(hipMemcpyAsync(c.ptr.p, r.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
      GRB_HIP_TRY(hipMemcpyAsync(c.ind.p, r.ind.p, 4 * (size_t)En, hipMemcpyDeviceToDevice, s));
      GRB_HIP_TRY(hipMemcpyAsync(c.val.p, r.val.p, 4 * (size_t)En, hipMemcpyDeviceToDevice, s));
    }
  } else {
    GRB_HIP_TRY(hipMemsetAsync(r.ptr.p, 0, 4 * ((size_t)n + 1), s));
    if (both) GRB_HIP_TRY(hipMemsetAsync(c.ptr.p, 0, 4 * ((size_t)n + 1), s));
  }
  GRB_HIP_TRY(hipStreamSynchronize(s));
  if (both) c.h_ptr = r.h_ptr;
  GRB_HIP_TRY(hipEventElapsedTime(&out.loop_ms, ev.a, ev.b));
  out.result_edges = En / 2;
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches C)
  GRB_TRY(attach(C, &r, both ? &c : nullptr));
  if (res) *res = out;
  return GRB_SUCCESS;
}

grb_info truss_check(grb_matrix C, grb_matrix A, int k) {
  if (!C || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  if (A->nrows != A->ncols || C->nrows != A->nrows || C->ncols != A->nrows) return GRB_DIMENSION_MISMATCH;
  if (k < 2) return GRB_INVALID_VALUE;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || (C->dtype != GRB_F32 && C->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (!A->csr.ptr || (!A->csc_alias && !A->csc.ptr)) return GRB_INVALID_OBJECT;   // a product result: no CSC of its own
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// k-truss and trussness: the contract is the comment in include/grb_hip.h
grb_info grb_ktruss(grb_matrix C, grb_matrix A, int k, grb_descriptor desc, grb_truss_result* result) { GRB_API_ENTER();
  (void)desc;
  GRB_TRY(truss_check(C, A, k));
  return truss_run(C, A, k, false, result);
}

grb_info grb_trussness(grb_matrix C, grb_matrix A, grb_descriptor desc, grb_truss_result* result) { GRB_API_ENTER();
  (void)desc;
  GRB_TRY(truss_check(C, A, 2));
  return truss_run(C, A, 3, true, result);
}
