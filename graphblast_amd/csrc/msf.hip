// msf.hip -- the minimum spanning forest on the device: grb_msf.  The contract is the comment in include/grb_hip.h; the
// reference has no such driver (graphblas/algorithm/), the definition is this project's own:
//   the forest Kruskal builds when it takes the edges in the order of the key (w, min(u, v), max(u, v)).
//
// Boruvka, and the whole loop is ONE co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid
// barrier between its passes); the host reads one record when it is over.
//   comp     i32 per vertex: the representative of the vertex's component (a vertex number).
//   parent   i32 per vertex, read at representatives: where the component hooked.
//   best     u64 per vertex, read at representatives: the smallest (ordered weight bits << 32 | min endpoint) among the
//            component's outgoing edges; best2, u32: among those that have it, the smallest max endpoint.
//   cand     i32 per vertex: the CSR position of the vertex's own best outgoing edge in this round, or kMsFin: every
//            neighbour shares its component (components only merge: it is never walked again).
//   forest   (vertex, CSR position) per forest edge, at most n - 1, appended through a per-wave LDS stage.
//   round    A  every unfinished vertex walks its row for the smallest key among the entries that leave its component and
//               gives it one 64-bit atomicMin at its component's slot.  For a fixed vertex v the order of (w, min, max) is
//               the order of (w, u), so a row's minimum is one 64-bit compare per entry.
//            B  the vertices whose candidate has the slot's key take a 32-bit atomicMin of the max endpoint.
//            C  exactly one vertex per component matches both: it owns the component's edge.  The other end's component d
//               chose the same edge exactly when its two slots hold the same key (a mutual pair): the smaller
//               representative stays root and appends the edge; otherwise the component hooks, parent = d, and appends it.
//            D  pointer jumping: a vertex follows up to kMsHops parents a pass and keeps the last; passes until every vertex
//               has found its root (at most kMsJumps).
//            E  comp = parent[comp]; the slots are reset.
//            The loop ends when no vertex has a candidate or a round appended nothing, after at most kMsRounds rounds.
//   labels   one atomicMin per vertex at its representative, then a relabelling pass: comp(v) = the smallest member.
//   rows     of up to kMsLaneLen entries: a lane, four entries in flight; up to kMsWaveLen: a wave, 16-byte index loads;
//            longer: the workgroup.  Pass A deals the vertices to the WAVES of the grid 64 at a time, neighbouring numbers to
//            different waves: a graph's hubs often have neighbouring numbers.
// After the loop the forest list is expanded to both directions as (row << 32 | column, value bits) pairs, ordered by the
// library's radix sort (a star's forest row is as long as the star, so rows are not sorted one by one), the pointers are a
// lower bound per row, and the weight is a two-level sum whose shape depends on the number of entries alone.
// Working memory: 56 bytes per vertex and 4.3 KiB (the state and the partial sums), one allocation; the sort brings 24
// more per vertex of its own.
#include "graph_common.hpp"

namespace grb {

constexpr int kMsLaneLen = 8;                            // a row of up to this many entries: one lane walks it
constexpr int kMsWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kMsStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kMsRounds = 32;                            // n < 2^31 halves at least that often; an asymmetric input stops here
constexpr int kMsHops = 16;                              // parents a vertex follows in one jumping pass
constexpr int kMsJumps = 40;                             // jumping passes a round: a hook chain of n components is flat after log_16 n + 1
constexpr int kMsRec = 16;
constexpr Index kMsFin = -2;
constexpr unsigned long long kMsNone = ~0ull;
constexpr int kMsSumBlocks = 256;                        // partial sums of the weight, at most

struct MsSlot {                     // what one pass adds up; 128 bytes
  unsigned a, b;
  unsigned long long sum;
  unsigned pad[28];
};
struct MsState {                    // zeroed by the host before the launch
  GridBarrier bar;
  MsSlot slot[4];                   // pass p adds into slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned forest[32];              // forest edges appended so far (only pass C adds, and everybody reads it before the next one)
  unsigned flag[32];                // the symmetry check (graph_common.hpp): 1 = the CSR and the CSC differ
  unsigned long long rec[kMsRec];   // [0] off-diagonal entries [1] forest edges [2] components [3] isolated [4] rounds [5] passes
                                    // [6] done [7] a NaN off the diagonal
};
constexpr int kMsDone = 6, kMsNan = 7;

struct MsArgs {
  const Index *ptr, *ind;
  const unsigned* val;              // the stored values' bits
  Index n;
  int f32;
  unsigned long long* best;
  unsigned* best2;
  int *comp, *parent;
  Index *cand, *fv, *fpos;
  MsState* st;
};

// ---- a wave's staged appends of (vertex, position) -------------------------------------------------------------------------
// cnt is the same in every lane; every lane of the wave calls these together
struct MsOut {
  Index *sv, *sp;                   // the wave's stage (LDS)
  unsigned cnt;                     // staged
  unsigned cap;                     // room in the list
};
__device__ __forceinline__ void ms_flush(const MsArgs& a, MsOut& o, int lane) {
  if (o.cnt == 0u) return;
  const unsigned cnt = o.cnt;
  __builtin_amdgcn_wave_barrier();
  unsigned at = 0;
  if (lane == 0) at = atomicAdd(&a.st->forest[0], cnt);
  at = (unsigned)__shfl((int)at, 0, kWave);
  for (unsigned i = (unsigned)lane; i < cnt; i += kWave)
    if (at + i < o.cap) {                                                    // (always on a symmetric input: a forest has n - 1 edges at most)
      publish(&a.fv[at + i], o.sv[i]);
      publish(&a.fpos[at + i], o.sp[i]);
    }
  __builtin_amdgcn_wave_barrier();
  o.cnt = 0u;
}
__device__ __forceinline__ void ms_push(const MsArgs& a, MsOut& o, int lane, bool want, Index v, Index pos) {
  const unsigned long long m = __ballot(want);
  if (m == 0ull) return;
  if (o.cnt + kWave > (unsigned)kMsStage) ms_flush(a, o, lane);
  if (want) {
    const unsigned at = o.cnt + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    o.sv[at] = v;
    o.sp[at] = pos;
  }
  o.cnt += (unsigned)__popcll(m);
}

// ---- up to N entries of v's row (v in component c): the component loads, then the value loads, then the compares -----------
template <int N>
__device__ __forceinline__ void ms_hit(const MsArgs& a, Index v, int c, const Index (&u)[N], const Index (&p)[N], bool (&ok)[N],
                                       unsigned long long& best, Index& bpos, bool& nan) {
  int cu[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n && u[j] != v;
    cu[j] = ok[j] ? fresh(&a.comp[u[j]]) : c;
  }
  unsigned w[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok[j] = ok[j] && cu[j] != c;
    w[j] = ok[j] ? a.val[p[j]] : 0u;
  }
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (ok[j]) {
      if (a.f32 && (w[j] & 0x7fffffffu) > 0x7f800000u) nan = true;
      const unsigned long long key = ((unsigned long long)weight_order(w[j], a.f32) << 32) | (unsigned)u[j];
      if (key < best) { best = key; bpos = p[j]; }
    }
}

// the row [b, e) of v walked by kThreads threads (t: this one's number among them)
template <int kThreads>
__device__ __forceinline__ void ms_walk(const MsArgs& a, Index v, int c, Index b, Index e, int t, unsigned long long& best, Index& bpos, bool& nan) {
  const QuadSpan s = quad_span(a.ind, b, e);
  const Index b4 = s.b4, nq = s.nq, te = s.te, nh = s.nh, ns = s.ns;
  if (kThreads == kWave || t < kWave) {
    Index u[1] = {0}, p[1] = {0};
    bool ok[1] = {t < ns};
    if (ok[0]) {
      p[0] = t < nh ? b + t : te + (t - nh);
      u[0] = a.ind[p[0]];
    }
    ms_hit<1>(a, v, c, u, p, ok, best, bpos, nan);
  }
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    bool ok[4];
    ok[0] = ok[1] = ok[2] = ok[3] = q < nq;
    const Index at = b4 + 4 * (ok[0] ? q : 0);
    const int4 w = ok[0] ? *reinterpret_cast<const int4*>(a.ind + at) : make_int4(0, 0, 0, 0);
    const Index u[4] = {w.x, w.y, w.z, w.w};
    const Index p[4] = {at, at + 1, at + 2, at + 3};
    ms_hit<4>(a, v, c, u, p, ok, best, bpos, nan);
  }
}

// v's row is walked: its candidate (key = ordered weight << 32 | other end), or none
__device__ __forceinline__ void ms_settle(const MsArgs& a, Index v, int c, unsigned long long key, Index pos, unsigned& ncand) {
  if (key == kMsNone) {
    publish(&a.cand[v], kMsFin);
    return;
  }
  publish(&a.cand[v], pos);
  const unsigned u = (unsigned)key, lo = u < (unsigned)v ? u : (unsigned)v;
  const unsigned long long k64 = (key & 0xffffffff00000000ull) | lo;
  if (fresh(&a.best[c]) > k64) atomicMin(&a.best[c], k64);                   // (the slot only falls: a large component's vertices mostly skip)
  ++ncand;
}

// the edge at position pos of v's row: the other end, the key's two parts
__device__ __forceinline__ bool ms_edge(const MsArgs& a, Index v, Index pos, Index& u, unsigned long long& k64, unsigned& mx) {
  u = a.ind[pos];
  if ((unsigned)u >= (unsigned)a.n) return false;
  const unsigned lo = (unsigned)(u < v ? u : v);
  mx = (unsigned)(u < v ? v : u);
  k64 = ((unsigned long long)weight_order(a.val[pos], a.f32) << 32) | lo;
  return true;
}

__global__ __launch_bounds__(kPThreads) void msf_persistent_kernel(MsArgs a) {
  __shared__ Index s_sv[kPWaves][kMsStage];
  __shared__ Index s_sp[kPWaves][kMsStage];
  __shared__ Index s_big[kPThreads];
  __shared__ int s_nbig;
  __shared__ unsigned long long s_key[kPWaves];
  __shared__ Index s_pos[kPWaves];
  __shared__ unsigned long long s_red[kPWaves][3];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  const long long gwave = (long long)wave * G + blockIdx.x, gwaves = (long long)G * kPWaves;   // neighbouring chunks: different CUs
  MsState* st = a.st;
  if (st->flag[0] != 0u) return;                         // not symmetric: every workgroup reads the same word
  const long long n = a.n;
  const unsigned cap = a.n > 0 ? (unsigned)a.n - 1u : 0u;
  MsOut o = {s_sv[wave], s_sp[wave], 0u, cap};
  unsigned gen = 0, passes = 0, rounds = 0, forest = 0;
  MsSlot* sl = &st->slot[0];

  // a pass begins: its slot, the one after the next cleared; and ends: the barrier
  auto pass_begin = [&]() {
    sl = &st->slot[passes & 3u];
    if (blockIdx.x == 0 && tid == 0) {
      MsSlot* z = &st->slot[(passes + 2u) & 3u];
      publish(&z->a, 0u);
      publish(&z->b, 0u);
      publish(&z->sum, 0ull);
    }
  };
  auto pass_end = [&]() -> bool {
    if (!grid_sync(&st->bar, gen, false)) return false;
    ++passes;
    return true;
  };
  // the workgroup's part of a pass's sums, one atomic each
  auto reduce = [&](unsigned x, unsigned y, unsigned long long sum) {
    x = wave_sum_u32(x);
    y = wave_sum_u32(y);
    sum = wave_sum_u64(sum);
    if (lane == 0) { s_red[wave][0] = x; s_red[wave][1] = y; s_red[wave][2] = sum; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long bx = 0, by = 0, bs = 0;
      for (int w = 0; w < kPWaves; ++w) { bx += s_red[w][0]; by += s_red[w][1]; bs += s_red[w][2]; }
      if (bx) __hip_atomic_fetch_add(&sl->a, (unsigned)bx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (by) __hip_atomic_fetch_add(&sl->b, (unsigned)by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bs) __hip_atomic_fetch_add(&sl->sum, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  // ---- pass 0: every vertex its own component; the degrees
  unsigned long long offdiag = 0;
  unsigned isolated = 0;
  {
    unsigned my_iso = 0;
    unsigned long long my_sum = 0;
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const int d = row_degree_no_diag(a.ptr, a.ind, (Index)v);
      publish(&a.comp[v], (int)v);
      publish(&a.parent[v], (int)v);
      publish(&a.best[v], kMsNone);
      publish(&a.best2[v], ~0u);
      publish(&a.cand[v], d == 0 ? kMsFin : (Index)0);
      my_sum += (unsigned long long)d;
      if (d == 0) ++my_iso;
    }
    reduce(my_iso, 0u, my_sum);
    if (!pass_end()) return;
    isolated = fresh(&sl->a);
    offdiag = fresh(&sl->sum);
  }

  bool nan_found = false;
  while (rounds < (unsigned)kMsRounds) {
    // ---- A: the candidates
    {
      unsigned ncand = 0;
      bool nan = false;
      pass_begin();
      for (long long base = 0; base < n; base += gwaves * kWave) {
        if (tid == 0) s_nbig = 0;
        __syncthreads();
        const long long vv = base + (long long)lane * gwaves + gwave;        // neighbouring numbers: different waves and CUs (hubs come in runs)
        Index v = 0, b = 0, e = 0;
        int c = 0;
        if (vv < n && fresh(&a.cand[vv]) != kMsFin) {
          v = (Index)vv;
          b = a.ptr[v];
          e = a.ptr[v + 1];
          c = fresh(&a.comp[v]);
          if (e <= b) publish(&a.cand[v], kMsFin);       // (never: it has an off-diagonal entry)
        }
        const Index len = e > b ? e - b : 0;
        if (len > kMsWaveLen) s_big[atomicAdd(&s_nbig, 1)] = v;              // (at most one a thread: room for all)
        {                                                                    // the short rows, a lane each
          const bool mine = len > 0 && len <= kMsLaneLen;
          const unsigned longest = wave_max_u32(mine ? (unsigned)len : 0u);
          unsigned long long key = kMsNone;
          Index pos = 0;
          for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
            Index u[4], p[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ok[j] = mine && j0 + j < len;
              p[j] = ok[j] ? b + j0 + j : 0;
              u[j] = ok[j] ? a.ind[p[j]] : 0;
            }
            ms_hit<4>(a, v, c, u, p, ok, key, pos, nan);
          }
          if (mine) ms_settle(a, v, c, key, pos, ncand);
        }
        unsigned long long mids = __ballot(len > kMsLaneLen && len <= kMsWaveLen);
        while (mids) {                                                       // the wave's rows, one after the other
          const int l = __ffsll((long long)mids) - 1;
          mids &= mids - 1ull;
          const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
          const int wc = __builtin_amdgcn_readlane(c, l);
          unsigned long long key = kMsNone;
          Index pos = 0;
          ms_walk<kWave>(a, wv, wc, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, key, pos, nan);
          const unsigned long long mn = wave_reduce(key, [](unsigned long long x, unsigned long long y) { return x < y ? x : y; });
          const unsigned long long who = __ballot(key == mn);
          pos = (Index)__shfl((int)pos, __ffsll((long long)who) - 1, kWave);
          if (lane == 0) ms_settle(a, wv, wc, mn, pos, ncand);
        }
        __syncthreads();
        const int nbig = s_nbig;
        for (int r = 0; r < nbig; ++r) {                                     // the workgroup's rows
          const Index w = s_big[r];
          const int wc = fresh(&a.comp[w]);
          unsigned long long key = kMsNone;
          Index pos = 0;
          ms_walk<kPThreads>(a, w, wc, a.ptr[w], a.ptr[w + 1], tid, key, pos, nan);
          const unsigned long long mn = wave_reduce(key, [](unsigned long long x, unsigned long long y) { return x < y ? x : y; });
          const unsigned long long who = __ballot(key == mn);
          pos = (Index)__shfl((int)pos, __ffsll((long long)who) - 1, kWave);
          if (lane == 0) { s_key[wave] = mn; s_pos[wave] = pos; }
          __syncthreads();
          if (tid == 0) {
            unsigned long long bk = s_key[0];
            Index bp = s_pos[0];
            for (int x = 1; x < kPWaves; ++x)
              if (s_key[x] < bk) { bk = s_key[x]; bp = s_pos[x]; }
            ms_settle(a, w, wc, bk, bp, ncand);
          }
          __syncthreads();
        }
        __syncthreads();
      }
      reduce(ncand, nan ? 1u : 0u, 0ull);
      if (!pass_end()) return;
      if (fresh(&sl->b) != 0u) { nan_found = true; break; }
      if (fresh(&sl->a) == 0u) break;
    }
    // ---- B: among a component's candidates with its key, the smallest max endpoint
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const Index pos = fresh(&a.cand[v]);
      if (pos < 0) continue;
      Index u;
      unsigned long long k64;
      unsigned mx;
      if (!ms_edge(a, (Index)v, pos, u, k64, mx)) continue;
      const int c = fresh(&a.comp[v]);
      if (fresh(&a.best[c]) == k64) atomicMin(&a.best2[c], mx);
    }
    if (!pass_end()) return;
    // ---- C: the owner of a component's edge hooks and appends
    pass_begin();
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      bool want = false;
      Index pos = v < n ? fresh(&a.cand[v]) : kMsFin;
      if (pos >= 0) {
        Index u;
        unsigned long long k64;
        unsigned mx;
        if (ms_edge(a, (Index)v, pos, u, k64, mx)) {
          const int c = fresh(&a.comp[v]);
          if (fresh(&a.best[c]) == k64 && fresh(&a.best2[c]) == mx) {
            const int d = fresh(&a.comp[u]);
            const bool mutual = fresh(&a.best[d]) == k64 && fresh(&a.best2[d]) == mx;
            if (mutual && c < d) {
              want = true;                                                   // the pair's root: it alone appends
            } else if (d != c) {
              publish(&a.parent[c], d);
              want = !mutual;
            }
          }
        }
      }
      ms_push(a, o, lane, want, (Index)v, pos);
    }
    ms_flush(a, o, lane);
    if (!pass_end()) return;
    ++rounds;
    {
      unsigned total = fresh(&st->forest[0]);
      if (total > cap) total = cap;
      const unsigned added = total - forest;
      forest = total;
      if (added == 0u) break;
    }
    // ---- D: pointer jumping to the fixpoint
    for (int it = 0; it < kMsJumps; ++it) {
      unsigned changed = 0;
      pass_begin();
      for (long long x = gtid; x < n; x += gthreads) {
        const int p0 = fresh(&a.parent[x]);
        if (p0 == (int)x) continue;
        int p = p0;
        bool root = false;
        for (int hop = 0; hop < kMsHops && !root; ++hop) {                   // (a parent only ever moves to an ancestor)
          const int pp = fresh(&a.parent[p]);
          root = pp == p;
          p = pp;
        }
        if (p != p0) publish(&a.parent[x], p);
        if (!root) ++changed;                                                // not there yet: another pass
      }
      reduce(changed, 0u, 0ull);
      if (!pass_end()) return;
      if (fresh(&sl->a) == 0u) break;
    }
    // ---- E: the new representatives; the slots for the next round
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const int c = fresh(&a.comp[v]);
      const int r = fresh(&a.parent[c]);
      if (r != c) publish(&a.comp[v], r);
      publish(&a.best[v], kMsNone);
      publish(&a.best2[v], ~0u);
    }
    if (!pass_end()) return;
  }

  unsigned comps = 0;
  if (!nan_found) {
    // ---- the labels: the smallest member of every component (best2 is all ones: pass 0 or the last pass E left it so)
    unsigned my_roots = 0;
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const int c = fresh(&a.comp[v]);
      if (fresh(&a.best2[c]) > (unsigned)v) atomicMin(&a.best2[c], (unsigned)v);
      if (c == (int)v) ++my_roots;
    }
    reduce(my_roots, 0u, 0ull);
    if (!pass_end()) return;
    comps = fresh(&sl->a);
    for (long long v = gtid; v < n; v += gthreads) a.comp[v] = (int)fresh(&a.best2[fresh(&a.comp[v])]);
  }
  if (gtid == 0) {
    st->rec[0] = offdiag;
    st->rec[1] = forest;
    st->rec[2] = comps;
    st->rec[3] = isolated;
    st->rec[4] = rounds;
    st->rec[5] = passes;
    st->rec[kMsNan] = nan_found ? 1ull : 0ull;
    st->rec[kMsDone] = 1ull;
  }
}

// ---- after the loop: the forest list as sorted (row << 32 | column, value bits) pairs, C's arrays, the weight ---------------
// the stored value is the one in the row of the smaller end (the two differ in the sign of a zero at most)
__global__ __launch_bounds__(kBlock) void ms_expand_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, const unsigned* __restrict__ val,
                                                           Index n, const Index* __restrict__ fv, const Index* __restrict__ fpos, long long F,
                                                           unsigned long long* __restrict__ keys, unsigned* __restrict__ pay) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < F; i += (long long)gridDim.x * kBlock) {
    Index v = fv[i];
    const Index pos = fpos[i];
    if ((unsigned)v >= (unsigned)n) v = 0;                                   // (never)
    Index u = ind[pos];
    if ((unsigned)u >= (unsigned)n) u = v;                                   // (never)
    unsigned w = val[pos];
    if (u < v) {                                                             // v's twin entry in row u
      const Index e = ptr[u + 1], lo = index_lower_bound(ind, ptr[u], e, v);
      if (lo < e && ind[lo] == v) w = val[lo];
    }
    keys[2 * i] = ((unsigned long long)(unsigned)v << 32) | (unsigned)u;
    keys[2 * i + 1] = ((unsigned long long)(unsigned)u << 32) | (unsigned)v;
    pay[2 * i] = w;
    pay[2 * i + 1] = w;
  }
}

// the pointers: a lower bound per row; the indices and the values
__global__ __launch_bounds__(kBlock) void ms_rows_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ pay, long long m,
                                                         long long n1, Index* __restrict__ optr, Index* __restrict__ oind, unsigned* __restrict__ oval) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n1 + m; i += (long long)gridDim.x * kBlock) {
    if (i < n1) {
      const unsigned long long want = (unsigned long long)i << 32;
      long long lo = 0, hi = m;
      while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
      }
      optr[i] = (Index)lo;
    } else {
      oind[i - n1] = (Index)(unsigned)keys[i - n1];
      oval[i - n1] = pay[i - n1];
    }
  }
}

// the weight over the entries above the diagonal, each edge once: block b adds the entries b * kBlock + t + k * blocks * kBlock in
// the order of k; the rest of the sum is graph_common.hpp's fixed-order tail (weight_block_sum, weight_final_kernel)
template <bool kF32>
__global__ __launch_bounds__(kBlock) void ms_weight_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ pay, long long m,
                                                           unsigned long long* __restrict__ partial) {
  double fs = 0.0;
  long long is = 0;
  for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < m; j += (long long)gridDim.x * kBlock) {
    const unsigned long long k = keys[j];
    if ((unsigned)k > (unsigned)(k >> 32)) {
      if (kF32) fs += (double)__uint_as_float(pay[j]);
      else is += (long long)(int)pay[j];
    }
  }
  weight_block_sum<kF32>(fs, is, partial);
}

namespace {

grb_info msf_run(grb_matrix C, grb_vector comp, grb_matrix A, grb_msf_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  const int f32 = A->dtype == GRB_F32 ? 1 : 0;
  const bool both = C->format != 1;
  grb_msf_result r = {};
  Side sr, sc;
  if (n > 0) GRB_TRY(persistent_kernel_fits<msf_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, best (8 bytes), six words per vertex, then the pairs of both directions and the partial sums
  const size_t st_bytes = pad_bytes(sizeof(MsState));
  const size_t vw = pad_words((size_t)n);
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 56 * vw + 8 * (size_t)kMsSumBlocks + 64));
  MsArgs a;
  a.ptr = A->csr.ptr;
  a.ind = A->csr.ind;
  a.val = (const unsigned*)A->csr.val;
  a.n = n;
  a.f32 = f32;
  a.st = (MsState*)work.p;
  a.best = (unsigned long long*)((char*)work.p + st_bytes);
  a.best2 = (unsigned*)(a.best + vw);
  a.comp = (int*)(a.best2 + vw);
  a.parent = a.comp + vw;
  a.cand = (Index*)(a.parent + vw);
  a.fv = a.cand + vw;
  a.fpos = a.fv + vw;
  unsigned long long* d_keys = (unsigned long long*)(a.fpos + vw);           // [2 vw]
  unsigned* d_pay = (unsigned*)(d_keys + 2 * vw);                            // [2 vw]
  unsigned long long* d_partial = (unsigned long long*)(d_pay + 2 * vw);     // [kMsSumBlocks]
  double* d_weight = (double*)(d_partial + kMsSumBlocks);
  if (comp) GRB_TRY(dense_out_prepare(comp, n));         // before anything runs; comp stays as it was until the end
  long long F = 0;
  if (n > 0) {
    GRB_TRY(bfs_lanes_fence(s));    // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
    GRB_HIP_TRY(hipEventRecord(ev.a, s));
    GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
    launch_symmetry_check<true>(A, &a.st->flag[0], s);
    hipLaunchKernelGGL(msf_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
    GRB_HIP_TRY(hipGetLastError());
    struct { unsigned flag[32]; unsigned long long rec[kMsRec]; } h;
    GRB_HIP_TRY(hipMemcpyAsync(&h, a.st->flag, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the call's one read of the loop
    if (h.flag[0] != 0u) return GRB_INVALID_VALUE;       // A's CSR and CSC differ: not symmetric
    if (h.rec[kMsDone] != 1ull) return GRB_PANIC;        // a grid barrier gave up
    if (h.rec[kMsNan] != 0ull) return GRB_INVALID_VALUE; // a NaN off the diagonal
    F = (long long)h.rec[1];
    if (F > (long long)n - 1) F = (long long)n - 1;
    r.edges = (int64_t)(h.rec[0] / 2);
    r.forest_edges = (int64_t)F;
    r.components = (int32_t)h.rec[2];
    r.isolated = (int32_t)h.rec[3];
    r.rounds = (int32_t)h.rec[4];
    r.passes = (int32_t)h.rec[5];
    r.launches = 1;
  }
  // ---- C's arrays
  const long long m = 2 * F;
  GRB_TRY(side_alloc(&sr, n, m));
  if (both) GRB_TRY(side_alloc(&sc, n, m));
  if (m > 0) {
    hipLaunchKernelGGL(ms_expand_kernel, dim3(stream_grid(F)), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, (const unsigned*)A->csr.val, n,
                       a.fv, a.fpos, F, d_keys, d_pay);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_sort_pairs(d_keys, d_pay, m, key_bits(n), key_bits(n)));
    hipLaunchKernelGGL(ms_rows_kernel, dim3(stream_grid((long long)n + 1 + m)), dim3(kBlock), 0, s, d_keys, d_pay, m, (long long)n + 1,
                       (Index*)sr.ptr.p, (Index*)sr.ind.p, (unsigned*)sr.val.p);
    const int blocks = (int)((m + kBlock - 1) / kBlock < kMsSumBlocks ? (m + kBlock - 1) / kBlock : kMsSumBlocks);
    if (f32) {
      hipLaunchKernelGGL(ms_weight_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, d_keys, d_pay, m, d_partial);
      hipLaunchKernelGGL(weight_final_kernel<true>, dim3(1), dim3(kWave), 0, s, d_partial, blocks, d_weight);
    } else {
      hipLaunchKernelGGL(ms_weight_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, d_keys, d_pay, m, d_partial);
      hipLaunchKernelGGL(weight_final_kernel<false>, dim3(1), dim3(kWave), 0, s, d_partial, blocks, d_weight);
    }
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(&r.weight, d_weight, 8, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    if (both) GRB_TRY(side_mirror(&sc, sr, n, m, s));    // the structure is symmetric and so are the values: the CSC is a copy
  } else {
    GRB_HIP_TRY(hipMemsetAsync(sr.ptr.p, 0, 4 * ((size_t)n + 1), s));
    if (both) GRB_HIP_TRY(hipMemsetAsync(sc.ptr.p, 0, 4 * ((size_t)n + 1), s));
  }
  if (n > 0) {
    GRB_HIP_TRY(hipEventRecord(ev.b, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
    GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  } else {
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  if (both) sc.h_ptr = sr.h_ptr;
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches C) and two copies.  A, which
  // may be C, has been read for the last time
  GRB_TRY(attach(C, &sr, both ? &sc : nullptr));
  if (comp) GRB_TRY(dense_out_commit(comp, a.comp, n, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_msf(grb_matrix C, grb_vector comp, grb_matrix A, grb_descriptor desc, grb_msf_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!C || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || C->nrows != n || C->ncols != n || (comp && comp->nsize != n)) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || (comp && comp->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (C->dtype != A->dtype) return GRB_DOMAIN_MISMATCH;
  if (n > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return msf_run(C, comp, A, result);
}
