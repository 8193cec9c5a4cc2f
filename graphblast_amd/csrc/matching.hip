// matching.hip -- greedy weighted and maximal matching on the device: grb_matching.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definition is this project's own:
//   the matching the greedy scan builds when it takes the edges in the order of the key (p, min(u, v), max(u, v)) and keeps
//   an edge when both ends are still free; p is the weight descending, ascending, or a hash of the two ends and a seed.
//
// The locally dominant edge algorithm: an edge that is the best live edge at both of its ends is in the greedy matching of
// what is left.  The whole loop is ONE co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid
// barrier between its passes); the host reads one record when it is over.
//   mate     i32 per vertex: the partner, or -1.
//   cand     i32 per vertex: the other end of the vertex's best live entry, or kMtFin: no neighbour is free (neighbours only
//            get matched: it is never walked again); cpos: that entry's CSR position.
//   queue    the vertices to evaluate in this round; list: the matched vertices in the order they were found (each once).
//   round    A  every queued vertex walks its row for the smallest (ordered p << 32 | other end) among the entries whose other
//               end has no partner.  For a fixed vertex the order of (p, min, max) is the order of (p, other end).  The
//               walker owns cand(v): no atomic.  Round 0 takes every vertex with an off-diagonal entry.
//            B  every evaluated v with cand(cand(v)) = v is matched.  Either end or both may see the pair (the other end may
//               have kept its candidate from an earlier round): each end is claimed by a compare-and-swap of mate from -1,
//               and whoever wins it appends it to the list, so a vertex enters the list exactly once.
//            C  every newly matched x walks its row and queues each free neighbour y with cand(y) = x.  y has one candidate,
//               so it is queued once.  A vertex whose candidate is still free keeps it and is not walked again.
//            The loop ends when the queue is empty or a round matched nothing (that bounds an asymmetric input), after at
//            most n / 2 + 1 rounds.
//   rows     of up to kMtLaneLen entries: a lane, four entries in flight; up to kMtWaveLen: a wave, 16-byte index loads;
//            longer: the workgroup.  The items of a pass are dealt to the WAVES of the grid 64 at a time, neighbouring ones to
//            different waves, as in msf.hip.
// After the loop C has at most one entry a row and needs no sort: pointers = a scan of (mate >= 0), index = mate, value = the
// bits at cpos of the smaller end.  The weight is a two-level sum over the vertices with mate(v) > v whose shape depends on
// n alone.  Working memory: 24 bytes per vertex and about 3 KiB (the state, the scan's totals, the partial sums), one
// allocation.
#include "graph_common.hpp"

namespace grb {

constexpr int kMtLaneLen = 8;                            // a row of up to this many entries: one lane walks it
constexpr int kMtWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kMtStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kMtRec = 16;
constexpr Index kMtFree = -1;                            // mate: no partner
constexpr Index kMtFin = -2;                             // cand: no free neighbour, for good
constexpr unsigned long long kMtNone = ~0ull;
constexpr int kMtSumBlocks = 256;                        // partial sums of the weight, at most

struct MtSlot {                     // what one pass adds up; 128 bytes
  unsigned a, b;
  unsigned long long sum;
  unsigned pad[28];
};
struct MtState {                    // zeroed by the host before the launch
  GridBarrier bar;
  MtSlot slot[4];                   // pass p adds into slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned queued[2][32];           // round r evaluates queued[r & 1][0] vertices; its pass C counts the next round's in the other
  unsigned matched[32];             // vertices in the list so far (only pass B adds)
  unsigned flag[32];                // the symmetry check (graph_common.hpp): 1 = the CSR and the CSC differ
  unsigned long long rec[kMtRec];   // [0] off-diagonal entries [1] matched vertices [2] isolated [3] rounds [4] passes
                                    // [5] evaluations [6] done [7] a NaN off the diagonal
};
constexpr int kMtDone = 6, kMtNan = 7;

struct MtArgs {
  const Index *ptr, *ind;
  const unsigned* val;              // the stored values' bits
  Index n;
  int f32, mode;
  unsigned seed;
  int* mate;
  Index *cand, *cpos, *queue, *list;
  MtState* st;
};

// p of the edge {v, u} whose stored bits are w: the smaller goes first
__device__ __forceinline__ unsigned mt_prio(const MtArgs& a, Index v, Index u, unsigned w) {
  if (a.mode == GRB_MATCH_HASHED) {
    const unsigned lo = (unsigned)(u < v ? u : v), hi = (unsigned)(u < v ? v : u);
    return hash_mix32(hash_mix32(lo + a.seed) ^ hi);                        // (graph_common.hpp)
  }
  const unsigned o = weight_order(w, a.f32);
  return a.mode == GRB_MATCH_HEAVIEST ? ~o : o;
}

// ---- what a pass does with the entries of a row -----------------------------------------------------------------------------
// pass A: the smallest key among the entries whose other end is free
struct MtBest {
  static constexpr bool kBest = true;
  const MtArgs& a;
  bool first;                       // round 0: every vertex that is not finished
  bool nan;
  __device__ __forceinline__ bool wanted(Index v) const { return !first || fresh(&a.cand[v]) != kMtFin; }
  template <int N>
  __device__ __forceinline__ void hit(Index v, const Index (&u)[N], const Index (&p)[N], bool (&ok)[N], unsigned long long& best, Index& bpos) {
    int mu[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n && u[j] != v;
      mu[j] = ok[j] && !first ? fresh(&a.mate[u[j]]) : (int)kMtFree;         // (round 0: nobody has a partner yet)
    }
    unsigned w[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && mu[j] == kMtFree;
      w[j] = ok[j] && a.mode != GRB_MATCH_HASHED ? a.val[p[j]] : 0u;
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (ok[j]) {
        if (a.f32 && a.mode != GRB_MATCH_HASHED && (w[j] & 0x7fffffffu) > 0x7f800000u) nan = true;
        const unsigned long long key = ((unsigned long long)mt_prio(a, v, u[j], w[j]) << 32) | (unsigned)u[j];
        if (key < best) { best = key; bpos = p[j]; }
      }
  }
  __device__ __forceinline__ void settle(Index v, unsigned long long key, Index pos) {
    if (key == kMtNone) {
      publish(&a.cand[v], kMtFin);
      return;
    }
    publish(&a.cpos[v], pos);
    publish(&a.cand[v], (Index)(unsigned)key);
  }
};
// pass C: the free neighbours whose candidate is the newly matched vertex go to the queue
struct MtWake {
  static constexpr bool kBest = false;
  const MtArgs& a;
  WaveStage& o;
  int lane;
  __device__ __forceinline__ bool wanted(Index) const { return true; }
  template <int N>
  __device__ __forceinline__ void hit(Index v, const Index (&u)[N], const Index (&)[N], bool (&ok)[N], unsigned long long&, Index&) {
    int mu[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n && u[j] != v;
      mu[j] = ok[j] ? fresh(&a.mate[u[j]]) : 0;
    }
    Index cu[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && mu[j] == kMtFree;
      cu[j] = ok[j] ? fresh(&a.cand[u[j]]) : kMtFin;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) stage_push<kMtStage>(o, lane, ok[j] && cu[j] == v, u[j]);  // (every lane of the wave is here)
  }
  __device__ __forceinline__ void settle(Index, unsigned long long, Index) {}
};

// the row [b, e) of v walked by kThreads threads (t: this one's number among them); whole waves call it together
template <int kThreads, typename Op>
__device__ __forceinline__ void mt_walk(Op& op, const Index* ind, Index v, Index b, Index e, int t, unsigned long long& best, Index& bpos) {
  const QuadSpan s = quad_span(ind, b, e);
  const Index b4 = s.b4, nq = s.nq, te = s.te, nh = s.nh, ns = s.ns;
  if (kThreads == kWave || t < kWave) {
    Index u[1] = {0}, p[1] = {0};
    bool ok[1] = {t < ns};
    if (ok[0]) {
      p[0] = t < nh ? b + t : te + (t - nh);
      u[0] = ind[p[0]];
    }
    op.template hit<1>(v, u, p, ok, best, bpos);
  }
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    bool ok[4];
    ok[0] = ok[1] = ok[2] = ok[3] = q < nq;
    const Index at = b4 + 4 * (ok[0] ? q : 0);
    const int4 w = ok[0] ? *reinterpret_cast<const int4*>(ind + at) : make_int4(0, 0, 0, 0);
    const Index u[4] = {w.x, w.y, w.z, w.w};
    const Index p[4] = {at, at + 1, at + 2, at + 3};
    op.template hit<4>(v, u, p, ok, best, bpos);
  }
}

struct MtLds {
  Index big[kPThreads];             // the batch's rows for the workgroup
  int nbig;
  unsigned long long key[kPWaves];
  Index pos[kPWaves];
};

// the rows of `count` vertices (list[i], or i itself without a list), by their length classes; the whole grid calls it together
template <typename Op>
__device__ __forceinline__ void mt_rows(const MtArgs& a, Op& op, long long count, const Index* list, MtLds& L, int tid, int lane, int wave,
                                        long long gwave, long long gwaves) {
  auto least = [](unsigned long long x, unsigned long long y) { return x < y ? x : y; };
  for (long long base = 0; base < count; base += gwaves * kWave) {
    if (tid == 0) L.nbig = 0;
    __syncthreads();
    const long long i = base + (long long)lane * gwaves + gwave;             // neighbouring items: different waves and CUs (hubs come in runs)
    Index v = 0, b = 0, e = 0;
    if (i < count) {
      const Index x = list ? fresh(&list[i]) : (Index)i;
      if ((unsigned)x < (unsigned)a.n && op.wanted(x)) {
        v = x;
        b = a.ptr[v];
        e = a.ptr[v + 1];
        if (e <= b) op.settle(v, kMtNone, 0);            // (never: it has an off-diagonal entry)
      }
    }
    const Index len = e > b ? e - b : 0;
    if (len > kMtWaveLen) L.big[atomicAdd(&L.nbig, 1)] = v;                  // (at most one a thread: room for all)
    {                                                                        // the short rows, a lane each
      const bool mine = len > 0 && len <= kMtLaneLen;
      const unsigned longest = wave_max_u32(mine ? (unsigned)len : 0u);
      unsigned long long key = kMtNone;
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
        op.template hit<4>(v, u, p, ok, key, pos);
      }
      if (mine) op.settle(v, key, pos);
    }
    unsigned long long mids = __ballot(len > kMtLaneLen && len <= kMtWaveLen);
    while (mids) {                                                           // the wave's rows, one after the other
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
      unsigned long long key = kMtNone;
      Index pos = 0;
      mt_walk<kWave>(op, a.ind, wv, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, key, pos);
      if (Op::kBest) {
        const unsigned long long mn = wave_reduce(key, least);
        const unsigned long long who = __ballot(key == mn);
        pos = (Index)__shfl((int)pos, __ffsll((long long)who) - 1, kWave);
        if (lane == 0) op.settle(wv, mn, pos);
      }
    }
    __syncthreads();
    const int nbig = L.nbig;
    for (int r = 0; r < nbig; ++r) {                                         // the workgroup's rows
      const Index w = L.big[r];
      unsigned long long key = kMtNone;
      Index pos = 0;
      mt_walk<kPThreads>(op, a.ind, w, a.ptr[w], a.ptr[w + 1], tid, key, pos);
      if (Op::kBest) {
        const unsigned long long mn = wave_reduce(key, least);
        const unsigned long long who = __ballot(key == mn);
        pos = (Index)__shfl((int)pos, __ffsll((long long)who) - 1, kWave);
        if (lane == 0) { L.key[wave] = mn; L.pos[wave] = pos; }
        __syncthreads();
        if (tid == 0) {
          unsigned long long bk = L.key[0];
          Index bp = L.pos[0];
          for (int x = 1; x < kPWaves; ++x)
            if (L.key[x] < bk) { bk = L.key[x]; bp = L.pos[x]; }
          op.settle(w, bk, bp);
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPThreads) void matching_persistent_kernel(MtArgs a) {
  __shared__ Index s_stage[kPWaves][kMtStage];
  __shared__ MtLds s_rows;
  __shared__ unsigned long long s_red[kPWaves][3];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  const long long gwave = (long long)wave * G + blockIdx.x, gwaves = (long long)G * kPWaves;   // neighbouring chunks: different CUs
  MtState* st = a.st;
  if (st->flag[0] != 0u) return;                         // not symmetric: every workgroup reads the same word
  const long long n = a.n;
  unsigned gen = 0, passes = 0, rounds = 0, total = 0;
  unsigned long long evaluations = 0;
  MtSlot* sl = &st->slot[0];

  // a pass begins: its slot, the one after the next cleared; and ends: the barrier
  auto pass_begin = [&]() {
    sl = &st->slot[passes & 3u];
    if (blockIdx.x == 0 && tid == 0) {
      MtSlot* z = &st->slot[(passes + 2u) & 3u];
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

  // ---- pass 0: nobody has a partner; the degrees
  unsigned long long offdiag = 0;
  unsigned isolated = 0;
  {
    unsigned my_iso = 0;
    unsigned long long my_sum = 0;
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const int d = row_degree_no_diag(a.ptr, a.ind, (Index)v);
      publish(&a.mate[v], (int)kMtFree);
      publish(&a.cand[v], d == 0 ? kMtFin : kMtFree);
      publish(&a.cpos[v], (Index)0);
      my_sum += (unsigned long long)d;
      if (d == 0) ++my_iso;
    }
    reduce(my_iso, 0u, my_sum);
    if (!pass_end()) return;
    isolated = fresh(&sl->a);
    offdiag = fresh(&sl->sum);
  }

  bool nan_found = false;
  long long count = n;                                   // the vertices to evaluate: round 0 takes all that have a neighbour
  const unsigned long long max_rounds = (unsigned long long)n / 2ull + 1ull;
  while ((unsigned long long)rounds < max_rounds) {
    const Index* queue = rounds == 0u ? nullptr : a.queue;
    // ---- A: the candidates
    {
      MtBest op = {a, rounds == 0u, false};
      pass_begin();
      mt_rows(a, op, count, queue, s_rows, tid, lane, wave, gwave, gwaves);
      reduce(0u, op.nan ? 1u : 0u, 0ull);
      if (!pass_end()) return;
      evaluations += rounds == 0u ? (unsigned long long)(n - (long long)isolated) : (unsigned long long)count;
      if (fresh(&sl->b) != 0u) { nan_found = true; break; }
    }
    // ---- B: the pairs that chose each other
    {
      WaveStage o = {s_stage[wave], 0u, a.list, &st->matched[0], 0u, (unsigned)a.n};
      pass_begin();
      if (blockIdx.x == 0 && tid == 0) publish(&st->queued[rounds & 1u][0], 0u);   // (read by everybody before pass A; next added to in the next round's pass C)
      for (long long base = 0; base < count; base += gthreads) {
        const long long i = base + gtid;
        Index v = 0, u = 0;
        bool pv = false, pu = false;
        if (i < count) {
          const Index x = queue ? fresh(&queue[i]) : (Index)i;
          if ((unsigned)x < (unsigned)a.n) {
            const Index c = fresh(&a.cand[x]);
            if ((unsigned)c < (unsigned)a.n && fresh(&a.cand[c]) == x) {
              v = x;
              u = c;
              pv = atomicCAS(&a.mate[v], (int)kMtFree, (int)u) == (int)kMtFree;
              pu = atomicCAS(&a.mate[u], (int)kMtFree, (int)v) == (int)kMtFree;
            }
          }
        }
        stage_push<kMtStage>(o, lane, pv, v);
        stage_push<kMtStage>(o, lane, pu, u);
      }
      stage_flush(o, lane);
      if (!pass_end()) return;
    }
    ++rounds;
    unsigned now = fresh(&st->matched[0]);
    if (now > (unsigned)a.n) now = (unsigned)a.n;
    const unsigned before = total;
    total = now;
    if (total == before) break;                          // a round that matched nothing: the last
    // ---- C: the neighbours that lost their candidate
    {
      WaveStage o = {s_stage[wave], 0u, a.queue, &st->queued[rounds & 1u][0], 0u, (unsigned)a.n};
      MtWake op = {a, o, lane};
      pass_begin();
      mt_rows(a, op, (long long)(total - before), a.list + before, s_rows, tid, lane, wave, gwave, gwaves);
      stage_flush(o, lane);
      if (!pass_end()) return;
    }
    unsigned next = fresh(&st->queued[rounds & 1u][0]);
    if (next > (unsigned)a.n) next = (unsigned)a.n;
    count = (long long)next;
    if (count == 0) break;
  }

  if (gtid == 0) {
    st->rec[0] = offdiag;
    st->rec[1] = total;
    st->rec[2] = isolated;
    st->rec[3] = rounds;
    st->rec[4] = passes;
    st->rec[5] = evaluations;
    st->rec[kMtNan] = nan_found ? 1ull : 0ull;
    st->rec[kMtDone] = 1ull;
  }
}

// ---- after the loop: C's arrays and the weight -------------------------------------------------------------------------------
// flags[v] = 1 when v has a partner (v < n), flags[n] = 0: their exclusive scan is C's pointer array
__global__ __launch_bounds__(kBlock) void mt_flags_kernel(const int* __restrict__ mate, long long n, unsigned* __restrict__ flags) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v <= n; v += (long long)gridDim.x * kBlock)
    flags[v] = v < n && mate[v] >= 0 ? 1u : 0u;
}
// the one entry of a matched row: the partner and the bits stored in the row of the smaller end (its candidate's position)
__global__ __launch_bounds__(kBlock) void mt_fill_kernel(const int* __restrict__ mate, const Index* __restrict__ cpos, const unsigned* __restrict__ val,
                                                         long long n, long long m, const Index* __restrict__ optr, Index* __restrict__ oind,
                                                         unsigned* __restrict__ oval) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    const int u = mate[v];
    if (u < 0 || (long long)u >= n) continue;
    const long long at = optr[v];
    if (at < 0 || at >= m) continue;                                         // (never)
    oind[at] = (Index)u;
    oval[at] = val[cpos[(long long)u < v ? u : v]];
  }
}

// the weight over the vertices with mate(v) > v, each edge once: block b adds the vertices b * kBlock + t + k * blocks * kBlock in
// the order of k; the rest of the sum is graph_common.hpp's fixed-order tail (weight_block_sum, weight_final_kernel)
template <bool kF32>
__global__ __launch_bounds__(kBlock) void mt_weight_kernel(const int* __restrict__ mate, const Index* __restrict__ cpos, const unsigned* __restrict__ val,
                                                           long long n, unsigned long long* __restrict__ partial) {
  double fs = 0.0;
  long long is = 0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    const int u = mate[v];
    if ((long long)u > v) {
      const unsigned w = val[cpos[v]];
      if (kF32) fs += (double)__uint_as_float(w);
      else is += (long long)(int)w;
    }
  }
  weight_block_sum<kF32>(fs, is, partial);
}

namespace {

grb_info matching_run(grb_vector mate, grb_matrix C, grb_matrix A, int mode, unsigned seed, grb_matching_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  const int f32 = A->dtype == GRB_F32 ? 1 : 0;
  const bool both = C && C->format != 1;
  grb_matching_result r = {};
  Side sr, sc;
  if (n > 0) GRB_TRY(persistent_kernel_fits<matching_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, six words per vertex (mate, cand, cpos, queue, list, the flags of the scan), the scan's
  // totals, the partial sums and the weight
  const size_t st_bytes = pad_bytes(sizeof(MtState));
  const size_t vw = pad_words((size_t)n + 1);
  const size_t scan_bytes = (device_scan_u32_scratch((long long)n + 1) + 63) & ~(size_t)63;   // (to 64 bytes: d_partial is 8-byte words)
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 24 * vw + scan_bytes + 8 * (size_t)kMtSumBlocks + 64));
  MtArgs a;
  a.ptr = A->csr.ptr;
  a.ind = A->csr.ind;
  a.val = (const unsigned*)A->csr.val;
  a.n = n;
  a.f32 = f32;
  a.mode = mode;
  a.seed = seed;
  a.st = (MtState*)work.p;
  a.mate = (int*)((char*)work.p + st_bytes);
  a.cand = (Index*)(a.mate + vw);
  a.cpos = a.cand + vw;
  a.queue = a.cpos + vw;
  a.list = a.queue + vw;
  unsigned* d_flags = (unsigned*)(a.list + vw);                               // [n + 1]
  unsigned* d_totals = d_flags + vw;
  unsigned long long* d_partial = (unsigned long long*)((char*)d_totals + scan_bytes);   // [kMtSumBlocks]
  double* d_weight = (double*)(d_partial + kMtSumBlocks);
  GRB_TRY(dense_out_prepare(mate, n));                   // before anything runs; mate stays as it was until the end
  long long M = 0;                                       // matched vertices = C's entries
  if (n > 0) {
    GRB_TRY(bfs_lanes_fence(s));    // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
    GRB_HIP_TRY(hipEventRecord(ev.a, s));
    GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
    if (mode != GRB_MATCH_HASHED) launch_symmetry_check<true>(A, &a.st->flag[0], s);
    else launch_symmetry_check<false>(A, &a.st->flag[0], s);                  // (a hashed priority never reads the values)
    hipLaunchKernelGGL(matching_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
    GRB_HIP_TRY(hipGetLastError());
    struct { unsigned flag[32]; unsigned long long rec[kMtRec]; } h;
    GRB_HIP_TRY(hipMemcpyAsync(&h, a.st->flag, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the call's one read of the loop
    if (h.flag[0] != 0u) return GRB_INVALID_VALUE;       // A's CSR and CSC differ: not symmetric
    if (h.rec[kMtDone] != 1ull) return GRB_PANIC;        // a grid barrier gave up
    if (h.rec[kMtNan] != 0ull) return GRB_INVALID_VALUE; // a NaN off the diagonal
    M = (long long)h.rec[1];
    if (M > (long long)n) M = (long long)n;
    r.edges = (int64_t)(h.rec[0] / 2);
    r.matched = (int64_t)(M / 2);
    r.isolated = (int32_t)h.rec[2];
    r.exposed = (int32_t)((long long)n - (long long)h.rec[2] - M);
    r.rounds = (int32_t)h.rec[3];
    r.passes = (int32_t)h.rec[4];
    r.evaluations = (int32_t)(h.rec[5] > 0x7fffffffull ? 0x7fffffffull : h.rec[5]);
    r.launches = 1;
  }
  // ---- C's arrays
  if (C) {
    GRB_TRY(side_alloc(&sr, n, M));
    if (both) GRB_TRY(side_alloc(&sc, n, M));
  }
  if (M > 0) {
    const int blocks = (int)(((long long)n + kBlock - 1) / kBlock < kMtSumBlocks ? ((long long)n + kBlock - 1) / kBlock : kMtSumBlocks);
    if (f32) {
      hipLaunchKernelGGL(mt_weight_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, a.mate, a.cpos, a.val, (long long)n, d_partial);
      hipLaunchKernelGGL(weight_final_kernel<true>, dim3(1), dim3(kWave), 0, s, d_partial, blocks, d_weight);
    } else {
      hipLaunchKernelGGL(mt_weight_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, a.mate, a.cpos, a.val, (long long)n, d_partial);
      hipLaunchKernelGGL(weight_final_kernel<false>, dim3(1), dim3(kWave), 0, s, d_partial, blocks, d_weight);
    }
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(&r.weight, d_weight, 8, hipMemcpyDeviceToHost, s));
  }
  if (C && M > 0) {
    hipLaunchKernelGGL(mt_flags_kernel, dim3(stream_grid((long long)n + 1)), dim3(kBlock), 0, s, a.mate, (long long)n, d_flags);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_exclusive_scan_u32_async(d_flags, (long long)n + 1, d_totals));
    GRB_HIP_TRY(hipMemcpyAsync(sr.ptr.p, d_flags, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(mt_fill_kernel, dim3(stream_grid((long long)n)), dim3(kBlock), 0, s, a.mate, a.cpos, a.val, (long long)n, M,
                       (const Index*)sr.ptr.p, (Index*)sr.ind.p, (unsigned*)sr.val.p);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    if (both) GRB_TRY(side_mirror(&sc, sr, n, M, s));    // the structure is symmetric and so are the values: the CSC is a copy
  } else if (C) {
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
  if (C) GRB_TRY(attach(C, &sr, both ? &sc : nullptr));
  GRB_TRY(dense_out_commit(mate, a.mate, n, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_matching(grb_vector mate, grb_matrix C, grb_matrix A, int mode, uint32_t seed, grb_descriptor desc,
                      grb_matching_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!mate || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || mate->nsize != n || (C && (C->nrows != n || C->ncols != n))) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || mate->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  if (C && C->dtype != A->dtype) return GRB_DOMAIN_MISMATCH;
  if (mode != GRB_MATCH_HEAVIEST && mode != GRB_MATCH_LIGHTEST && mode != GRB_MATCH_HASHED) return GRB_INVALID_VALUE;
  if (n > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return matching_run(mate, C, A, mode, seed, result);
}
