// maxflow.hip -- maximum flow and minimum cut on the device: grb_maxflow.  The contract is the comment in include/grb_hip.h;
// the reference has no such driver (graphblas/algorithm/), LAGraph ships the algorithm as LAGr_MaxFlow.
//
// Synchronous push-relabel with exact global relabeling.  Plain launches build the residual structure; the whole loop is ONE
// co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid barrier between its passes); plain
// launches make the outputs; the host reads one record.
//   R        the residual structure: row v = the other ends of v's off-diagonal arcs in either direction, ascending (the union
//            of row v of A and column v of A, merged as lcc.hip merges them).  Every row starts at a multiple of four slots
//            and is filled up to one with kMfPad, so that a row is read 16 bytes a lane.  Per slot: the other end, the
//            residual capacity (u32: two antiparallel arcs of 2^31 - 1 fit), the twin slot in the other end's row, the
//            position in A or -1 for a pure reverse arc.
//   state    per vertex: the excess at the start of the round (i64, written by its owner alone), what it received during the
//            round (u64, integer atomicAdd), two height arrays, a stamp (the number of the queue the vertex is in), two queues
//            and the list of this round's receivers.
//   round    push     every queued u walks its row in stored order against the heights and its excess as they stood at the
//                     start of the round and pushes min(rest of the excess, residual) over every arc with h(u) = h(v) + 1.
//                     Only one direction of an arc pair can be admissible under one snapshot of the heights, so the pusher
//                     alone writes the pair's two residuals.  The first adder of a round (the atomicAdd returned 0) appends
//                     the receiver to the list unless its stamp says it is in the queue anyway.
//            relabel  every evaluated vertex and every receiver adds what it received to its excess; an evaluated vertex
//                     that still has excess takes 1 + the smallest height over its residual arcs, read from this round's
//                     array, written to the next round's; whoever has excess goes into the next queue.
//            The queue's order is whatever the atomics hand out; every decision reads the round's snapshot, so the residuals,
//            excesses and heights after a round do not depend on it.
//   relabel  globally: a level-synchronous backward BFS from the sink over residual arcs (exact heights), with F asked a
//            second one from the source offset by n; the rest gets the limit (n without F, 2n with it) and is never
//            evaluated.  It runs before the first round and whenever the evaluations since the last one reach n: a function
//            of the inputs and the round alone.
//   rows     of up to kMfLaneLen slots: a lane; up to kMfWaveLen: a wave, 256 slots a step; longer: the workgroup.  In the
//            wave's and the workgroup's push the stored-order rule is an exclusive prefix sum of the admissible residuals.
// The loop ends when the queue is empty: without F no vertex with excess has a height below n (none can reach the sink:
// the preflow is maximum), with F no vertex but the terminals has excess (the preflow is a flow).  value = the sink's excess;
// side = the last backward BFS from the sink.
// Working memory: 44 bytes per vertex, 16 bytes per slot of R (at most 2 nvals + 3 n slots) and with F 4 bytes per entry of
// A, one allocation.  R is proportional to nvals: the reverse arcs and the residuals have to live somewhere.
#include "graph_common.hpp"

namespace grb {

constexpr int kMfLaneLen = 8;                            // a row of up to this many slots: one lane walks it
constexpr int kMfWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kMfStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kMfRec = 16;
constexpr Index kMfPad = 0x7fffffff;                     // the other end of a slot that fills a row up: nobody's id
constexpr Index kMfUnset = -1;                           // a BFS label: not reached
constexpr unsigned kMfNone = 0xffffffffu;
constexpr unsigned long long kMfMaxSlots = 0x7fffffffull;

struct MfSlot {                     // what one pass counts; 128 bytes
  unsigned a, b;                    // a: appends to the next queue or frontier; b: to the list of receivers
  unsigned pad[30];
};
struct MfState {                    // zeroed by the host before the first kernel
  GridBarrier bar;
  MfSlot slot[4];                   // pass p counts in slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned flag[32];                // bit 0: a bad capacity
  unsigned long long total[4];      // [0] slots of R [1] stored off-diagonal entries of A
  unsigned long long rec[kMfRec];   // [0] value [1] rounds [2] global relabels [3] passes [4] done [5] sink side [6] cut arcs
                                    // [7] cut capacity [8] flow arcs
};
constexpr int kMfValue = 0, kMfRounds = 1, kMfRelabels = 2, kMfPasses = 3, kMfDone = 4, kMfSinkSide = 5, kMfCutArcs = 6, kMfCutCap = 7,
              kMfFlowArcs = 8;

struct MfArgs {
  const Index* rptr;                // [n + 1]
  const Index* oth;                 // per slot: the other end
  unsigned* cap;                    //           the residual capacity
  const Index* twin;                //           the slot of the reverse arc
  Index n, source, sink;
  long long slots;                  // room in the per-slot arrays
  int want_flow;
  long long* exc;
  unsigned long long* inc;
  Index *h0, *h1;
  unsigned* stamp;                  // after the loop: side
  Index *qa, *qb, *rl;
  MfState* st;
};

// the capacity of a stored value: mode 1: 1 and nothing is read; mode 0: i32 >= 0, f32 an integer value in 0 .. 2^24
__device__ __forceinline__ unsigned mf_capacity(const unsigned* __restrict__ val, Index at, int f32, int unit, bool* bad) {
  if (unit) return 1u;
  const unsigned b = val[at];
  if (!f32) {
    if ((int)b < 0) { *bad = true; return 0u; }
    return b;
  }
  const float f = __uint_as_float(b);
  if (!(f >= 0.0f && f <= 16777216.0f) || f != truncf(f)) { *bad = true; return 0u; }   // (a NaN fails the first test)
  return (unsigned)f;
}

// ---- R: the merged rows (lcc.hip's merge: an entry's slot = the kept entries of its own list before it + those of the other
// list below it that are not in both).  kFill false: deg[v] = the row's slots, filled up to a multiple of four, and the
// totals.  kFill true: deg has been scanned into rptr and row v is written.
template <bool kFill>
__global__ __launch_bounds__(kBlock) void mf_merge_kernel(const Index* __restrict__ rptr, const Index* __restrict__ rind,
                                                          const unsigned* __restrict__ rval, const Index* __restrict__ cptr,
                                                          const Index* __restrict__ cind, Index n, int f32, int unit, long long slots,
                                                          unsigned* __restrict__ sptr, Index* __restrict__ oth, unsigned* __restrict__ cap,
                                                          Index* __restrict__ apos, MfState* st) {
  const int lane = lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  if (kFill && st->total[0] > kMfMaxSlots) return;                       // (the scan has wrapped: nothing is written)
  unsigned long long my_slots = 0, my_arcs = 0;
  bool bad = false;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const Index rb = rptr[v], re = rptr[v + 1];
    const Index cb = cptr[v], ce = cptr[v + 1];
    const Index dr = index_lower_bound(rind, rb, re, (Index)v);             // where the diagonal lies, if stored
    const bool has_r = dr < re && rind[dr] == (Index)v;
    const Index dc = index_lower_bound(cind, cb, ce, (Index)v);
    const bool has_c = dc < ce && cind[dc] == (Index)v;
    const long long base = kFill ? (long long)sptr[v] : 0;
    const unsigned room = kFill ? sptr[v + 1] - sptr[v] : 0u;
    unsigned both = 0;                                                   // entries in both lists, before this step
    for (Index x0 = rb; x0 < re; x0 += kWave) {
      const Index x = x0 + lane;
      const Index u = x < re ? rind[x] : (Index)v;
      const bool keep = x < re && u != (Index)v;
      Index pc = cb;
      bool found = false;
      if (keep) {
        pc = index_lower_bound(cind, cb, ce, u);
        found = pc < ce && cind[pc] == u;
      }
      const unsigned long long bm = __ballot(found);
      if (kFill && keep) {
        const unsigned pos = (unsigned)(x - rb) - (has_r && dr < x ? 1u : 0u) + (unsigned)(pc - cb) - (has_c && dc < pc ? 1u : 0u) -
                             (both + (unsigned)__popcll(bm & below));
        const unsigned c = mf_capacity(rval, x, f32, unit, &bad);
        if (pos < room && base + pos < slots) {
          oth[base + pos] = u;
          cap[base + pos] = c;
          apos[base + pos] = x;
        }
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
        if (pos < room && base + pos < slots) {
          oth[base + pos] = w;
          cap[base + pos] = 0u;
          apos[base + pos] = -1;
        }
      }
      both += (unsigned)__popcll(bm);
    }
    const unsigned arcs = (unsigned)(re - rb) - (has_r ? 1u : 0u);
    const unsigned d = arcs + (unsigned)(ce - cb) - (has_c ? 1u : 0u) - nboth;
    const unsigned padded = (d + 3u) & ~3u;
    if (!kFill) {
      if (lane == 0) sptr[v] = padded;
      my_slots += padded;
      my_arcs += arcs;
    } else {
      for (unsigned k = d + (unsigned)lane; k < padded && k < room; k += kWave)
        if (base + k < slots) {
          oth[base + k] = kMfPad;
          cap[base + k] = 0u;
          apos[base + k] = -1;
        }
    }
  }
  if (!kFill && lane == 0) {
    if (my_slots) atomicAdd(&st->total[0], my_slots);
    if (my_arcs) atomicAdd(&st->total[1], my_arcs);
    if (blockIdx.x == 0 && threadIdx.x == 0) sptr[n] = 0u;
  }
  if (kFill && __ballot(bad) != 0ull && lane == 0) atomicOr(&st->flag[0], 1u);
}

// twin[p] = the slot of v in the row of the other end of slot p of row v (rows ascending, the fill sorts last)
__global__ __launch_bounds__(kBlock) void mf_twin_kernel(const Index* __restrict__ rptr, const Index* __restrict__ oth, Index n, long long slots,
                                                         Index* __restrict__ twin, const MfState* st) {
  if (st->total[0] > kMfMaxSlots) return;
  const int lane = lane_id();
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const Index b = rptr[v], e = rptr[v + 1];
    for (long long p = (long long)b + lane; p < (long long)e && p < slots; p += kWave) {
      const Index w = oth[p];
      Index t = -1;
      if ((unsigned)w < (unsigned)n) {
        const Index wb = rptr[w], we = rptr[w + 1];
        if (wb >= 0 && (long long)we <= slots) {
          const Index at = index_lower_bound(oth, wb, we, (Index)v);
          if (at < we && oth[at] == (Index)v) t = at;
        }
      }
      twin[p] = t;
    }
  }
}

struct MfLds {
  Index big[kPThreads];             // the batch's rows for the workgroup
  int nbig;
  unsigned key[kPWaves];
  unsigned long long wtot[kPWaves];
};

// what a pass of the loop needs besides the arguments
struct MfRound {
  const Index* hc;                  // this round's heights
  Index* hn;                        // the next round's
  Index limit;                      // a vertex at this height or above is not evaluated
  unsigned qid;                     // the number of this round's queue
};

// d units go over slot p of u's row to v; c is the slot's residual.  true: v is to be appended to the receivers
__device__ __forceinline__ bool mf_move(const MfArgs& a, const MfRound& r, Index p, Index v, unsigned c, unsigned d) {
  publish(&a.cap[p], c - d);
  const Index tp = a.twin[p];
  if (tp >= 0 && (long long)tp < a.slots) publish(&a.cap[tp], fresh(&a.cap[tp]) + d);
  const unsigned long long old = __hip_atomic_fetch_add(&a.inc[v], (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return old == 0ull && fresh(&a.stamp[v]) != r.qid;
}

// the push over the row [b, e) of u by kThreads threads (t: this one's number among them); whole waves call it together.
// A step is a quad of slots a thread; the threads' admissible residuals before this one are an exclusive prefix sum.
template <int kThreads>
__device__ __forceinline__ void mf_push_walk(const MfArgs& a, const MfRound& r, WaveStage& o, MfLds& L, Index u, Index hu, unsigned long long e0,
                                             Index b, Index e, int t, int lane, int wave) {
  const Index nq = (e - b) >> 2;
  unsigned long long rem = e0;
  for (Index q0 = 0; q0 < nq && rem > 0ull; q0 += kThreads) {
    const Index q = q0 + t;
    const bool ok = q < nq;
    const Index at = b + 4 * (ok ? q : 0);
    const int4 w = ok ? *reinterpret_cast<const int4*>(a.oth + at) : make_int4(kMfPad, kMfPad, kMfPad, kMfPad);
    const Index v[4] = {w.x, w.y, w.z, w.w};
    Index hv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) hv[j] = (unsigned)v[j] < (unsigned)a.n ? fresh(&r.hc[v[j]]) : hu;
    unsigned adm[4];
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      adm[j] = (unsigned)v[j] < (unsigned)a.n && hu == hv[j] + 1 ? fresh(&a.cap[at + j]) : 0u;
      s += adm[j];
    }
    const unsigned long long incl = wave_incl_scan_u64(s);
    unsigned long long pre = incl - s, tot = __shfl(incl, kWave - 1, kWave);
    if (kThreads > kWave) {
      if (lane == 0) L.wtot[wave] = tot;
      __syncthreads();
      tot = 0;
      for (int x = 0; x < kPWaves; ++x) {
        const unsigned long long wt = L.wtot[x];
        if (x < wave) pre += wt;
        tot += wt;
      }
      __syncthreads();
    }
    unsigned long long avail = rem > pre ? rem - pre : 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned d = (unsigned long long)adm[j] < avail ? adm[j] : (unsigned)avail;
      avail -= d;
      bool first = false;
      if (d > 0u) first = mf_move(a, r, at + j, v[j], adm[j], d);
      stage_push<kMfStage>(o, lane, first, v[j]);
    }
    rem -= rem < tot ? rem : tot;
  }
  if (t == 0) publish(&a.exc[u], (long long)rem);
}

// the push pass over `count` queued vertices; the whole grid calls it together
__device__ __forceinline__ void mf_push_rows(const MfArgs& a, const MfRound& r, WaveStage& o, long long count, const Index* queue, MfLds& L, int tid,
                                             int lane, int wave, long long gwave, long long gwaves) {
  for (long long base = 0; base < count; base += gwaves * kWave) {
    if (tid == 0) L.nbig = 0;
    __syncthreads();
    const long long i = base + (long long)lane * gwaves + gwave;             // neighbouring items: different waves and CUs
    Index u = 0, b = 0, e = 0, hu = 0;
    unsigned long long e0 = 0;
    if (i < count) {
      const Index x = fresh(&queue[i]);
      if ((unsigned)x < (unsigned)a.n) {
        const Index h = fresh(&r.hc[x]);
        const long long ex = fresh(&a.exc[x]);
        const Index rb = a.rptr[x], re = a.rptr[x + 1];
        if (h < r.limit && ex > 0 && rb >= 0 && re > rb && (long long)re <= a.slots) {
          u = x; hu = h; e0 = (unsigned long long)ex; b = rb; e = re;
        }
      }
    }
    const Index len = e - b;
    if (len > kMfWaveLen) L.big[atomicAdd(&L.nbig, 1)] = u;                  // (at most one a thread: room for all)
    {                                                                        // the short rows, a lane each, in stored order
      const bool mine = len > 0 && len <= kMfLaneLen;
      const unsigned longest = wave_max_u32(mine ? (unsigned)len : 0u);
      unsigned long long rem = mine ? e0 : 0ull;
      for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
        const bool okq = mine && j0 < len;
        const int4 w = okq ? *reinterpret_cast<const int4*>(a.oth + b + j0) : make_int4(kMfPad, kMfPad, kMfPad, kMfPad);
        const Index v[4] = {w.x, w.y, w.z, w.w};
        Index hv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = (unsigned)v[j] < (unsigned)a.n ? fresh(&r.hc[v[j]]) : hu;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bool first = false;
          if ((unsigned)v[j] < (unsigned)a.n && hu == hv[j] + 1 && rem > 0ull) {
            const unsigned c = fresh(&a.cap[b + j0 + j]);
            const unsigned d = (unsigned long long)c < rem ? c : (unsigned)rem;
            if (d > 0u) {
              first = mf_move(a, r, b + j0 + j, v[j], c, d);
              rem -= d;
            }
          }
          stage_push<kMfStage>(o, lane, first, v[j]);
        }
      }
      if (mine) publish(&a.exc[u], (long long)rem);
    }
    unsigned long long mids = __ballot(len > kMfLaneLen && len <= kMfWaveLen);
    while (mids) {                                                           // the wave's rows, one after the other
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wu = (Index)__builtin_amdgcn_readlane((int)u, l);
      const Index whu = (Index)__builtin_amdgcn_readlane((int)hu, l);
      const unsigned long long we0 = __shfl(e0, l, kWave);
      mf_push_walk<kWave>(a, r, o, L, wu, whu, we0, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane,
                          lane, wave);
    }
    __syncthreads();
    const int nbig = L.nbig;
    for (int k = 0; k < nbig; ++k) {                                         // the workgroup's rows
      const Index w = L.big[k];
      const Index whu = fresh(&r.hc[w]);
      const long long wex = fresh(&a.exc[w]);                                // (read by all before thread 0 writes it: the walk has barriers)
      __syncthreads();
      mf_push_walk<kPThreads>(a, r, o, L, w, whu, (unsigned long long)wex, a.rptr[w], a.rptr[w + 1], tid, lane, wave);
      __syncthreads();
    }
    __syncthreads();
  }
}

// ---- what the other passes do with the slots of a row -------------------------------------------------------------------------
// the relabel pass: the smallest height over the residual arcs
struct MfLabel {
  static constexpr bool kBest = true;
  const MfArgs& a;
  const MfRound& r;
  WaveStage& o;
  // x was evaluated in this round: its excess, its height in the next round's array; true: it is relabelled and queued
  __device__ __forceinline__ bool wanted(Index x) const {
    const unsigned long long got = fresh(&a.inc[x]);
    long long ex = fresh(&a.exc[x]);
    if (got) {
      ex += (long long)got;
      publish(&a.exc[x], ex);
      publish(&a.inc[x], 0ull);
    }
    const Index h = fresh(&r.hc[x]);
    const bool go = ex > 0 && h < r.limit && x != a.source && x != a.sink;
    if (!go) publish(&r.hn[x], h);
    else publish(&a.stamp[x], r.qid + 1u);
    return go;
  }
  template <int N>
  __device__ __forceinline__ void hit(Index, const Index (&u)[N], const Index (&p)[N], bool (&ok)[N], unsigned& best, int) {
    unsigned c[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n;
      c[j] = ok[j] ? fresh(&a.cap[p[j]]) : 0u;
    }
    Index h[N];
#pragma unroll
    for (int j = 0; j < N; ++j) h[j] = ok[j] && c[j] > 0u ? fresh(&r.hc[u[j]]) : (Index)0x7fffffff;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((unsigned)h[j] < best) best = (unsigned)h[j];
  }
  __device__ __forceinline__ void settle(Index v, unsigned best) {
    // excess came in over an arc whose twin is residual, and a vertex with excess reaches the source: below 2 n, always
    if (best >= 2u * (unsigned)a.n) {
      publish(&a.st->bar.abort_flag[0], 1u);
      best = 2u * (unsigned)a.n;
    }
    publish(&r.hn[v], (Index)(best + 1u));
  }
};
// a level of the backward BFS: the other ends whose arc towards the frontier vertex has residual get the next label
struct MfBfs {
  static constexpr bool kBest = false;
  const MfArgs& a;
  WaveStage& o;
  Index* d;
  Index label;
  __device__ __forceinline__ bool wanted(Index) const { return true; }
  template <int N>
  __device__ __forceinline__ void hit(Index, const Index (&u)[N], const Index (&p)[N], bool (&ok)[N], unsigned&, int lane) {
    Index tp[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n;
      tp[j] = ok[j] ? a.twin[p[j]] : -1;
      ok[j] = ok[j] && tp[j] >= 0 && (long long)tp[j] < a.slots;
    }
    unsigned c[N];
#pragma unroll
    for (int j = 0; j < N; ++j) c[j] = ok[j] ? fresh(&a.cap[tp[j]]) : 0u;
    Index du[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      ok[j] = ok[j] && c[j] > 0u;
      du[j] = ok[j] ? fresh(&d[u[j]]) : 0;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool won = ok[j] && du[j] == kMfUnset && atomicCAS(&d[u[j]], kMfUnset, label) == kMfUnset;
      stage_push<kMfStage>(o, lane, won, u[j]);                                         // (every lane of the wave is here)
    }
  }
  __device__ __forceinline__ void settle(Index, unsigned) {}
};

// the row [b, e) of v walked by kThreads threads, a quad of slots each a step; whole waves call it together.  (R's rows begin
// and end on a 16-byte boundary: there is no head or tail, so graph_common.hpp's quad_span has nothing to do here)
template <int kThreads, typename Op>
__device__ __forceinline__ void mf_walk(Op& op, const Index* oth, Index v, Index b, Index e, int t, int lane, unsigned& best) {
  const Index nq = (e - b) >> 2;
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    bool ok[4];
    ok[0] = ok[1] = ok[2] = ok[3] = q < nq;
    const Index at = b + 4 * (ok[0] ? q : 0);
    const int4 w = ok[0] ? *reinterpret_cast<const int4*>(oth + at) : make_int4(0, 0, 0, 0);
    const Index u[4] = {w.x, w.y, w.z, w.w};
    const Index p[4] = {at, at + 1, at + 2, at + 3};
    op.template hit<4>(v, u, p, ok, best, lane);
  }
}

// the rows of `count` listed vertices by their length classes; the whole grid calls it together.  kQueue: the vertices the
// operation wants are appended to its list as well (the relabel pass: the next round's queue)
template <bool kQueue, typename Op>
__device__ __forceinline__ void mf_rows(const MfArgs& a, Op& op, long long count, const Index* list, MfLds& L, int tid, int lane, int wave,
                                        long long gwave, long long gwaves) {
  for (long long base = 0; base < count; base += gwaves * kWave) {
    if (tid == 0) L.nbig = 0;
    __syncthreads();
    const long long i = base + (long long)lane * gwaves + gwave;
    Index v = 0, b = 0, e = 0;
    bool go = false;
    if (i < count) {
      const Index x = fresh(&list[i]);
      if ((unsigned)x < (unsigned)a.n && op.wanted(x)) {
        go = true;
        v = x;
        const Index rb = a.rptr[x], re = a.rptr[x + 1];
        if (rb >= 0 && re > rb && (long long)re <= a.slots) { b = rb; e = re; }
        else if (Op::kBest) op.settle(v, kMfNone);                           // (never: it has excess, so it has an arc)
      }
    }
    if (kQueue) stage_push<kMfStage>(op.o, lane, go, v);
    const Index len = e - b;
    if (len > kMfWaveLen) L.big[atomicAdd(&L.nbig, 1)] = v;
    {                                                                        // the short rows, a lane each
      const bool mine = len > 0 && len <= kMfLaneLen;
      const unsigned longest = wave_max_u32(mine ? (unsigned)len : 0u);
      unsigned best = kMfNone;
      for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
        bool ok[4];
        ok[0] = ok[1] = ok[2] = ok[3] = mine && j0 < len;
        const Index at = ok[0] ? b + j0 : 0;
        const int4 w = ok[0] ? *reinterpret_cast<const int4*>(a.oth + at) : make_int4(0, 0, 0, 0);
        const Index u[4] = {w.x, w.y, w.z, w.w};
        const Index p[4] = {at, at + 1, at + 2, at + 3};
        op.template hit<4>(v, u, p, ok, best, lane);
      }
      if (mine) op.settle(v, best);
    }
    unsigned long long mids = __ballot(len > kMfLaneLen && len <= kMfWaveLen);
    while (mids) {                                                           // the wave's rows, one after the other
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
      unsigned best = kMfNone;
      mf_walk<kWave>(op, a.oth, wv, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, lane, best);
      if (Op::kBest) {
        best = wave_min_u32(best);
        if (lane == 0) op.settle(wv, best);
      }
    }
    __syncthreads();
    const int nbig = L.nbig;
    for (int k = 0; k < nbig; ++k) {                                         // the workgroup's rows
      const Index w = L.big[k];
      unsigned best = kMfNone;
      mf_walk<kPThreads>(op, a.oth, w, a.rptr[w], a.rptr[w + 1], tid, lane, best);
      if (Op::kBest) {
        best = wave_min_u32(best);
        if (lane == 0) L.key[wave] = best;
        __syncthreads();
        if (tid == 0) {
          unsigned bk = L.key[0];
          for (int x = 1; x < kPWaves; ++x)
            if (L.key[x] < bk) bk = L.key[x];
          op.settle(w, bk);
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPThreads) void maxflow_persistent_kernel(MfArgs a) {
  __shared__ Index s_stage[kPWaves][kMfStage];
  __shared__ MfLds s_rows;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  const long long gwave = (long long)wave * G + blockIdx.x, gwaves = (long long)G * kPWaves;   // neighbouring chunks: different CUs
  MfState* st = a.st;
  if (st->flag[0] != 0u || st->total[0] > kMfMaxSlots) return;               // a bad capacity, too many arcs: every workgroup reads the same words
  const long long n = a.n;
  const Index limit = a.want_flow ? (Index)(2 * n > 0x7ffffffell ? 0x7ffffffell : 2 * n) : a.n;
  unsigned gen = 0, passes = 0;
  MfSlot* sl = &st->slot[0];

  // a pass begins: its slot, the one after the next cleared; and ends: the barrier
  auto pass_begin = [&]() {
    sl = &st->slot[passes & 3u];
    if (blockIdx.x == 0 && tid == 0) {
      MfSlot* z = &st->slot[(passes + 2u) & 3u];
      publish(&z->a, 0u);
      publish(&z->b, 0u);
    }
  };
  auto pass_end = [&]() -> bool {
    if (!grid_sync(&st->bar, gen, false)) return false;
    ++passes;
    return true;
  };
  auto clamp_n = [&](unsigned x) -> long long { return x > (unsigned)a.n ? (long long)a.n : (long long)x; };

  // ---- nothing has excess, every height is 0
  pass_begin();
  for (long long v = gtid; v < n; v += gthreads) {
    publish(&a.exc[v], 0ll);
    publish(&a.inc[v], 0ull);
    publish(&a.h0[v], (Index)0);
    publish(&a.h1[v], (Index)0);
    publish(&a.stamp[v], 0u);
  }
  if (!pass_end()) return;
  // ---- the source's arcs are saturated (the other ends of a row are distinct: no atomic)
  pass_begin();
  {
    const Index b = a.rptr[a.source], e = a.rptr[a.source + 1];
    for (long long p = (long long)b + gtid; p < (long long)e && p < a.slots; p += gthreads) {
      const Index v = a.oth[p];
      if ((unsigned)v >= (unsigned)a.n) continue;
      const unsigned c = fresh(&a.cap[p]);
      const Index tp = a.twin[p];
      if (c == 0u || tp < 0 || (long long)tp >= a.slots) continue;
      publish(&a.cap[p], 0u);
      publish(&a.cap[tp], fresh(&a.cap[tp]) + c);
      publish(&a.exc[v], (long long)c);
    }
  }
  if (!pass_end()) return;

  Index *hc = a.h0, *hn = a.h1;                          // this round's heights, the next round's
  Index *qa = a.qa, *qb = a.qb;                          // this round's queue, the next round's
  unsigned qid = 0;
  long long count = 0;
  unsigned long long rounds = 0, relabels = 0, since = 0;
  // rounds: at most 2 n^2 with a relabel and 2 n^2 + 2 n without one (the highest active vertex sinks), and one more for every
  // vertex that leaves at the limit; the stamps are 32 bits
  unsigned long long max_rounds = 8ull * (unsigned long long)n * (unsigned long long)n + 4ull * (unsigned long long)n + 64ull;
  if (n > 0x10000 || max_rounds > 0x7ffffff0ull) max_rounds = 0x7ffffff0ull;

  // a backward BFS over residual arcs from the frontier of `fc` vertices in qa; d: the labels, the first new one `label`
  auto bfs = [&](Index* d, long long fc, Index label) -> bool {
    long long levels = 0;
    while (fc > 0 && levels <= n) {
      WaveStage o = {s_stage[wave], 0u, qb, &st->slot[passes & 3u].a, 0u, (unsigned)a.n};
      MfBfs op = {a, o, d, label};
      pass_begin();
      mf_rows<false>(a, op, fc, qa, s_rows, tid, lane, wave, gwave, gwaves);
      stage_flush(o, lane);
      if (!pass_end()) return false;
      fc = clamp_n(fresh(&sl->a));
      Index* t = qa; qa = qb; qb = t;
      ++label;
      ++levels;
    }
    return true;
  };
  // labels in d: the sink 0 and what reaches it; with `both` the source n and what reaches it; the rest unset
  auto label_all = [&](Index* d, bool both) -> bool {
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) publish(&d[v], v == a.sink ? (Index)0 : v == a.source ? a.n : kMfUnset);
    if (gtid == 0) publish(&qa[0], a.sink);
    if (!pass_end()) return false;
    if (!bfs(d, 1, 1)) return false;
    if (both) {
      pass_begin();
      if (gtid == 0) publish(&qa[0], a.source);
      if (!pass_end()) return false;
      if (!bfs(d, 1, a.n + 1)) return false;
    }
    return true;
  };

  bool dirty = true;                                     // a round has run since the last labels
  for (;;) {
    if (rounds == 0ull || since >= (unsigned long long)n) {
      // ---- global relabeling: exact heights in both arrays, the queue anew
      if (!label_all(hn, a.want_flow != 0)) return;
      ++qid;
      WaveStage o = {s_stage[wave], 0u, qa, &st->slot[passes & 3u].a, 0u, (unsigned)a.n};
      pass_begin();
      for (long long base = 0; base < n; base += gthreads) {
        const long long v = base + gtid;
        bool want = false;
        if (v < n) {
          const Index d = fresh(&hn[v]);
          const Index h = d == kMfUnset ? limit : d;
          publish(&hc[v], h);
          publish(&hn[v], h);
          want = h < limit && v != a.source && v != a.sink && fresh(&a.exc[v]) > 0;
          if (want) publish(&a.stamp[v], qid);
        }
        stage_push<kMfStage>(o, lane, want, (Index)v);
      }
      stage_flush(o, lane);
      if (!pass_end()) return;
      count = clamp_n(fresh(&sl->a));
      ++relabels;
      since = 0;
      dirty = false;
    }
    if (count == 0) break;
    if (rounds >= max_rounds) {
      if (gtid == 0) publish(&st->bar.abort_flag[0], 1u);
      return;
    }
    const MfRound r = {hc, hn, limit, qid};
    // ---- push
    {
      WaveStage o = {s_stage[wave], 0u, a.rl, &st->slot[passes & 3u].b, 0u, (unsigned)a.n};
      pass_begin();
      mf_push_rows(a, r, o, count, qa, s_rows, tid, lane, wave, gwave, gwaves);
      stage_flush(o, lane);
      if (!pass_end()) return;
    }
    const long long received = clamp_n(fresh(&sl->b));
    // ---- relabel, and the next round's queue
    {
      WaveStage o = {s_stage[wave], 0u, qb, &st->slot[passes & 3u].a, 0u, (unsigned)a.n};
      MfLabel op = {a, r, o};
      pass_begin();
      mf_rows<true>(a, op, count, qa, s_rows, tid, lane, wave, gwave, gwaves);
      for (long long base = 0; base < received; base += gthreads) {          // the receivers that were not evaluated
        const long long i = base + gtid;
        bool want = false;
        Index v = 0;
        if (i < received) {
          const Index x = fresh(&a.rl[i]);
          if ((unsigned)x < (unsigned)a.n) {
            v = x;
            const long long ex = fresh(&a.exc[x]) + (long long)fresh(&a.inc[x]);
            publish(&a.exc[x], ex);
            publish(&a.inc[x], 0ull);
            want = ex > 0 && x != a.source && x != a.sink && fresh(&hc[x]) < limit;
            if (want) publish(&a.stamp[x], qid + 1u);
          }
        }
        stage_push<kMfStage>(o, lane, want, v);
      }
      stage_flush(o, lane);
      if (!pass_end()) return;
    }
    since += (unsigned long long)count;
    count = clamp_n(fresh(&sl->a));
    { Index* t = qa; qa = qb; qb = t; }
    { Index* t = hc; hc = hn; hn = t; }
    ++qid;
    ++rounds;
    dirty = true;
  }

  // ---- side: what reaches the sink in the residual graph.  The labels of a global relabeling that no round followed are it
  if (dirty && !label_all(hn, false)) return;
  const Index* d = dirty ? hn : hc;
  pass_begin();
  for (long long v = gtid; v < n; v += gthreads) {
    const Index x = fresh(&d[v]);
    publish(&a.stamp[v], x != kMfUnset && x < a.n && v != a.source ? 1u : 0u);
  }
  if (!pass_end()) return;
  if (gtid == 0) {
    st->rec[kMfValue] = (unsigned long long)fresh(&a.exc[a.sink]);
    st->rec[kMfRounds] = rounds;
    st->rec[kMfRelabels] = relabels;
    st->rec[kMfPasses] = passes;
    st->rec[kMfDone] = 1ull;
  }
}

// ---- after the loop -----------------------------------------------------------------------------------------------------------
// One pass over A's entries by their slots: the cut (arcs from side 0 to side 1 and their capacities) and the sink side's
// size; kFlags: flags[position in A] = 1 where the flow max(0, capacity - residual) is positive; kWrite: F's entries.
template <bool kFlags, bool kWrite>
__global__ __launch_bounds__(kBlock) void mf_out_kernel(const Index* __restrict__ rptr, const Index* __restrict__ oth,
                                                        const unsigned* __restrict__ cap, const Index* __restrict__ apos,
                                                        const unsigned* __restrict__ aval, const unsigned* __restrict__ side, Index n,
                                                        long long slots, long long nvals, int f32, int unit, unsigned* __restrict__ flags,
                                                        Index* __restrict__ oind, unsigned* __restrict__ oval, long long m, MfState* st) {
  const int lane = lane_id();
  if (st->rec[kMfDone] != 1ull) return;
  unsigned long long cut_arcs = 0, cut_cap = 0, ones = 0;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < n; v += (long long)gridDim.x * kWavesPerBlock) {
    const Index b = rptr[v], e = rptr[v + 1];
    const unsigned sv = side[v];
    if (!kWrite && lane == 0) ones += sv;
    for (long long p = (long long)b + lane; p < (long long)e && p < slots; p += kWave) {
      const Index at = apos[p], u = oth[p];
      if (at < 0 || (long long)at >= nvals || (unsigned)u >= (unsigned)n) continue;
      bool bad = false;
      const unsigned c0 = mf_capacity(aval, at, f32, unit, &bad);
      const unsigned res = cap[p];
      const unsigned flow = c0 > res ? c0 - res : 0u;
      if (!kWrite) {
        if (sv == 0u && side[u] == 1u) { ++cut_arcs; cut_cap += c0; }
        if (kFlags && flow > 0u) flags[at] = 1u;
      } else if (flow > 0u) {
        const long long o = flags[at];                                       // (scanned: the entry's place in F)
        if (o < m) {
          oind[o] = u;
          oval[o] = f32 ? __float_as_uint((float)flow) : flow;
        }
      }
    }
  }
  if (!kWrite) {
    cut_arcs = wave_sum_u64(cut_arcs);
    cut_cap = wave_sum_u64(cut_cap);
    ones = wave_sum_u64(ones);
    if (lane == 0) {
      if (cut_arcs) atomicAdd(&st->rec[kMfCutArcs], cut_arcs);
      if (cut_cap) atomicAdd(&st->rec[kMfCutCap], cut_cap);
      if (ones) atomicAdd(&st->rec[kMfSinkSide], ones);
    }
  }
}
// F's pointers: the scanned flags at A's; and the number of F's entries into the record
__global__ __launch_bounds__(kBlock) void mf_ptr_kernel(const Index* __restrict__ aptr, const unsigned* __restrict__ flags, long long n,
                                                        long long nvals, Index* __restrict__ optr, MfState* st) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v <= n; v += (long long)gridDim.x * kBlock) {
    const long long at = aptr[v];
    optr[v] = (Index)flags[at < 0 ? 0 : at > nvals ? nvals : at];
    if (v == n) st->rec[kMfFlowArcs] = flags[nvals];
  }
}

namespace {

grb_info maxflow_run(grb_matrix F, grb_vector side, grb_matrix A, Index source, Index sink, int mode, grb_maxflow_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  const long long nvals = (long long)A->nvals;
  const int f32 = A->dtype == GRB_F32 ? 1 : 0;
  const int unit = mode == GRB_FLOW_UNIT ? 1 : 0;
  const bool both = F && F->format != 1;
  grb_maxflow_result r = {};
  Side sr, sc;
  GRB_TRY(persistent_kernel_fits<maxflow_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state; per vertex the row pointers, excess, received, two heights, stamp, two queues, receivers;
  // per slot of R four words (2 nvals + 3 n slots at most, and never more than INT32_MAX); the flags of F's scan; the totals
  // of the two scans
  unsigned long long slots_ull = 2ull * (unsigned long long)nvals + 3ull * (unsigned long long)n;
  if (slots_ull > kMfMaxSlots) slots_ull = kMfMaxSlots;
  const size_t slots = pad_words((size_t)slots_ull);
  const size_t st_bytes = pad_bytes(sizeof(MfState));
  const size_t vw = pad_words((size_t)n + 1);
  const size_t fw = F ? pad_words((size_t)nvals + 1) : 0;
  const size_t scan_n = (size_t)n + 1 > (size_t)nvals + 1 ? (size_t)n + 1 : (size_t)nvals + 1;
  const size_t scan_bytes = (device_scan_u32_scratch((long long)scan_n) + 63) & ~(size_t)63;   // (the last array: to 64 bytes)
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 16 * vw + 4 * 7 * vw + 16 * slots + 4 * fw + scan_bytes + 64));
  MfArgs a;
  a.st = (MfState*)work.p;
  a.exc = (long long*)((char*)work.p + st_bytes);
  a.inc = (unsigned long long*)(a.exc + vw);
  unsigned* d_rptr = (unsigned*)(a.inc + vw);
  a.rptr = (const Index*)d_rptr;
  a.h0 = (Index*)(d_rptr + vw);
  a.h1 = a.h0 + vw;
  a.stamp = (unsigned*)(a.h1 + vw);
  a.qa = (Index*)(a.stamp + vw);
  a.qb = a.qa + vw;
  a.rl = a.qb + vw;
  Index* d_oth = a.rl + vw;                              // (a multiple of 256 bytes from the start: the rows are read 16 bytes a lane)
  unsigned* d_cap = (unsigned*)(d_oth + slots);
  Index* d_twin = (Index*)(d_cap + slots);
  Index* d_apos = d_twin + slots;
  unsigned* d_flags = (unsigned*)(d_apos + slots);       // [nvals + 1] with F
  unsigned* d_totals = d_flags + fw;
  a.oth = d_oth;
  a.cap = d_cap;
  a.twin = d_twin;
  a.n = n;
  a.source = source;
  a.sink = sink;
  a.slots = (long long)slots_ull;
  a.want_flow = F ? 1 : 0;
  if (side) GRB_TRY(dense_out_prepare(side, n));         // before anything runs; side stays as it was until the end
  GRB_TRY(bfs_lanes_fence(s));      // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
  // ---- R
  const int wgrid = stream_grid((long long)n * kWave);
  hipLaunchKernelGGL(mf_merge_kernel<false>, dim3(wgrid), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, (const unsigned*)A->csr.val, A->csc.ptr,
                     A->csc.ind, n, f32, unit, a.slots, d_rptr, d_oth, d_cap, d_apos, a.st);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_async(d_rptr, (long long)n + 1, d_totals));
  hipLaunchKernelGGL(mf_merge_kernel<true>, dim3(wgrid), dim3(kBlock), 0, s, A->csr.ptr, A->csr.ind, (const unsigned*)A->csr.val, A->csc.ptr,
                     A->csc.ind, n, f32, unit, a.slots, d_rptr, d_oth, d_cap, d_apos, a.st);
  hipLaunchKernelGGL(mf_twin_kernel, dim3(wgrid), dim3(kBlock), 0, s, a.rptr, a.oth, n, a.slots, d_twin, a.st);
  GRB_HIP_TRY(hipGetLastError());
  // ---- the loop
  hipLaunchKernelGGL(maxflow_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
  GRB_HIP_TRY(hipGetLastError());
  // ---- the cut, and F's pointers
  if (F) {
    GRB_HIP_TRY(hipMemsetAsync(d_flags, 0, 4 * ((size_t)nvals + 1), s));
    hipLaunchKernelGGL((mf_out_kernel<true, false>), dim3(wgrid), dim3(kBlock), 0, s, a.rptr, a.oth, (const unsigned*)a.cap, (const Index*)d_apos,
                       (const unsigned*)A->csr.val, (const unsigned*)a.stamp, n, a.slots, nvals, f32, unit, d_flags, (Index*)nullptr,
                       (unsigned*)nullptr, 0ll, a.st);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_exclusive_scan_u32_async(d_flags, nvals + 1, d_totals));
    GRB_TRY(ewm_alloc(&sr.ptr, 4 * ((size_t)n + 1)));
    hipLaunchKernelGGL(mf_ptr_kernel, dim3(stream_grid((long long)n + 1)), dim3(kBlock), 0, s, A->csr.ptr, (const unsigned*)d_flags, (long long)n,
                       nvals, (Index*)sr.ptr.p, a.st);
  } else {
    hipLaunchKernelGGL((mf_out_kernel<false, false>), dim3(wgrid), dim3(kBlock), 0, s, a.rptr, a.oth, (const unsigned*)a.cap, (const Index*)d_apos,
                       (const unsigned*)A->csr.val, (const unsigned*)a.stamp, n, a.slots, nvals, f32, unit, (unsigned*)nullptr, (Index*)nullptr,
                       (unsigned*)nullptr, 0ll, a.st);
  }
  GRB_HIP_TRY(hipGetLastError());
  struct { unsigned flag[32]; unsigned long long total[4]; unsigned long long rec[kMfRec]; } h;
  GRB_HIP_TRY(hipMemcpyAsync(&h, a.st->flag, sizeof(h), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // the call's one read
  if (h.total[0] > kMfMaxSlots) return GRB_OUT_OF_MEMORY;   // more residual arcs than a 32-bit position can name (as grb_matrix_extract)
  if (h.flag[0] != 0u) return GRB_INVALID_VALUE;         // a capacity that is negative, fractional, not finite or above 2^24
  if (h.rec[kMfDone] != 1ull) return GRB_PANIC;          // a grid barrier gave up
  r.value = (int64_t)h.rec[kMfValue];
  r.arcs = (int64_t)h.total[1];
  r.flow_arcs = F ? (int64_t)h.rec[kMfFlowArcs] : -1;
  r.sink_side = (int64_t)h.rec[kMfSinkSide];
  r.cut_arcs = (int64_t)h.rec[kMfCutArcs];
  r.cut_capacity = (int64_t)h.rec[kMfCutCap];
  r.rounds = (int32_t)(h.rec[kMfRounds] > 0x7fffffffull ? 0x7fffffffull : h.rec[kMfRounds]);
  r.global_relabels = (int32_t)(h.rec[kMfRelabels] > 0x7fffffffull ? 0x7fffffffull : h.rec[kMfRelabels]);
  r.passes = (int32_t)(h.rec[kMfPasses] > 0x7fffffffull ? 0x7fffffffull : h.rec[kMfPasses]);
  r.launches = 1;
  // ---- F's entries
  if (F) {
    long long M = (long long)h.rec[kMfFlowArcs];
    if (M > nvals) M = nvals;
    GRB_TRY(ewm_alloc(&sr.ind, 4 * (size_t)(M > 0 ? M : 1)));
    GRB_TRY(ewm_alloc(&sr.val, 4 * (size_t)(M > 0 ? M : 1)));
    sr.nnz = (Index)M;
    sr.h_ptr.assign((size_t)n + 1, 0);
    if (M > 0) {
      hipLaunchKernelGGL((mf_out_kernel<false, true>), dim3(wgrid), dim3(kBlock), 0, s, a.rptr, a.oth, (const unsigned*)a.cap, (const Index*)d_apos,
                         (const unsigned*)A->csr.val, (const unsigned*)a.stamp, n, a.slots, nvals, f32, unit, d_flags, (Index*)sr.ind.p,
                         (unsigned*)sr.val.p, M, a.st);
      GRB_HIP_TRY(hipGetLastError());
    }
    GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
    if (both) {                                          // the CSC: the transpose of the CSR just made (the path behind grb_transpose)
      if (M > 0) {
        CsrArrays X;
        X.ptr = (Index*)sr.ptr.p;
        X.ind = (Index*)sr.ind.p;
        X.val = sr.val.p;
        X.n = n;
        X.nvals = (Index)M;
        GRB_TRY(transpose_side(X, n, n, &sc));
      } else {
        GRB_TRY(ewm_alloc(&sc.ptr, 4 * ((size_t)n + 1)));
        GRB_TRY(ewm_alloc(&sc.ind, 4));
        GRB_TRY(ewm_alloc(&sc.val, 4));
        GRB_HIP_TRY(hipMemsetAsync(sc.ptr.p, 0, 4 * ((size_t)n + 1), s));
        sc.h_ptr.assign((size_t)n + 1, 0);
        sc.nnz = 0;
      }
    }
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches F) and one copy.  A, which
  // may be F, has been read for the last time
  if (F) GRB_TRY(attach(F, &sr, both ? &sc : nullptr));
  if (side) GRB_TRY(dense_out_commit(side, a.stamp, n, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_maxflow(grb_matrix F, grb_vector side, grb_matrix A, int64_t source, int64_t sink, int mode, grb_descriptor desc,
                     grb_maxflow_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || (side && side->nsize != n) || (F && (F->nrows != n || F->ncols != n))) return GRB_DIMENSION_MISMATCH;
  if (source < 0 || source >= (int64_t)n || sink < 0 || sink >= (int64_t)n) return GRB_INDEX_OUT_OF_BOUNDS;
  if (source == sink || (mode != GRB_FLOW_CAPACITY && mode != GRB_FLOW_UNIT)) return GRB_INVALID_VALUE;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || (side && side->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (F && F->dtype != A->dtype) return GRB_DOMAIN_MISMATCH;
  if (!A->csr.ptr || A->csc_alias || !A->csc.ptr) return GRB_INVALID_OBJECT;   // a product result, the CSR-only format: no CSC of its own
  return maxflow_run(F, side, A, (Index)source, (Index)sink, mode, result);
}
