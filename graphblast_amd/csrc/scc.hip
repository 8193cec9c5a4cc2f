// scc.hip -- the strongly connected components on the device: grb_scc.  The contract is the comment in include/grb_hip.h;
// the reference has no such driver (graphblas/algorithm/), the definition is the textbook's:
//   scc(v) = the smallest vertex number among the vertices that reach v and are reached from v.
//
// The whole computation is ONE co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid barrier
// between its passes); the host reads one record when it is over.  Everything works on the LIVE vertices, those without a
// label yet.
//   state    u32 per vertex: bit 0 live, bit 1 F (reached from the pivot), bits 2 and 3 "queued for the next pass" of a
//            colouring (two, by the pass's parity: a pass sets one and clears the other, so no pass sets and clears one bit).
//            A vertex is REMOVED by the one atomic that clears its live bit and sees it set; that thread appends it.
//   din/dout i32 per vertex: the live in- and out-neighbours (column / row length minus a stored diagonal at first).  A
//            removed root's din counts its component.
//   colour   i32 per vertex: the colour of a round; once the vertex is removed, its label.
//   order    i32 per vertex: every vertex in the order of its removal.  order[rm, tail) are the removed vertices whose rows
//            and columns have not been walked yet; a trimming pass walks them (a returning atomic decrement of din of every
//            live out-neighbour and of dout of every live in-neighbour; the thread that sees 1 come back claims the vertex,
//            labels it with itself and appends it) and what it appends is the next pass's part.  live = n - tail, so
//            order[tail, n) has room for one frontier of live vertices; the sweeps below alternate between it and
//   qb       i32 per vertex: the other frontier of a sweep.
//   trim     pass 0 computes the degrees and removes what has none; trimming then runs to its fixpoint, and again after
//            every removal of components.
//   giant    the pivot is the live vertex with the largest din x dout (64 bits), the smallest number on a tie: two scans.
//            A forward sweep over rows sets F from the pivot; a backward sweep over columns that stays inside F removes
//            what it reaches, using order itself as its queue: that is the pivot's component.  Its smallest number is
//            taken along (a wave reduction, one atomic a wave) and written as the label of order's new part.
//   rounds   colour(v) = v on the live vertices, all of them queued; a pass gives every queued vertex's colour to its live
//            neighbours with atomicMin, and a neighbour whose colour dropped is queued once for the next pass.  At the
//            fixpoint the live vertices with colour(r) = r are the roots, each the smallest member of its component.  They
//            are removed and appended, and a sweep the other way that stays inside the colour removes the rest of every
//            root's component at once, again with order as its queue.  Even rounds colour along rows and collect along
//            columns, odd rounds the other way round.  The smallest live vertex is always a root, so a round removes at
//            least one component and n rounds bound the loop; the worst case is quadratic in passes.
//   rows     of up to kScLaneLen entries: a lane, four entries in flight; up to kScWaveLen: a wave, 16-byte index loads;
//            longer: the workgroup.  A pass deals its frontier to the WAVES of the grid, one vertex each while there are
//            more waves than vertices, else up to 64.
//   appends  are staged per wave in LDS, kScStage at a time, and reserved with one atomic per flush on the pass's own
//            counter (four slots in rotation, see kcore.hip for why a shared tail will not do).
// Working memory: state, din, dout, colour, order, qb: 24 bytes per vertex, and 2 KiB of state, one allocation.
#include <type_traits>
#include "graph_common.hpp"

namespace grb {

constexpr int kScLaneLen = 8;                            // a row of up to this many entries: one lane walks it
constexpr int kScWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kScStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kScRec = 16;
constexpr unsigned kScLive = 1u, kScF = 2u, kScQ0 = 4u, kScQ1 = 8u;

struct ScSlot {                     // what one pass adds up; 128 bytes
  unsigned added;                   // appended by the pass
  unsigned inv_min;                 // max of ~v (0: none)
  unsigned long long mx;
  unsigned long long sum;
  unsigned pad[26];
};
struct ScState {                    // zeroed by the host before the launch
  GridBarrier bar;
  ScSlot slot[4];                   // pass p adds into slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned giant_inv_min[32];       // max of ~v over the pivot's component
  unsigned long long rec[kScRec];   // [0] edges [1] components [2] largest [3] trivial [4] trimmed [5] rounds [6] passes [7] done
};
constexpr int kScDone = 7;

struct ScArgs {
  const Index *rptr, *rind;         // the CSR: out-edges
  const Index *cptr, *cind;         // the CSC: in-edges
  Index n;
  unsigned* state;
  int *din, *dout, *colour;
  Index *order, *qb;
  ScState* st;
};

enum { kScDecIn = 0, kScDecOut, kScFwd, kScBwd, kScProp, kScCollect };

// ---- what a pass does to the neighbour u (state word s) of its vertex v (colour c); true: this thread appends u -----------
template <int OP>
__device__ __forceinline__ bool sc_apply(const ScArgs& a, Index v, int c, unsigned qbit, Index u, unsigned s) {
  if (!(s & kScLive) || u == v) return false;
  if (OP == kScDecIn || OP == kScDecOut) {
    int* d = OP == kScDecIn ? a.din : a.dout;
    if (atomicSub(&d[u], 1) != 1) return false;
    if (!(atomicAnd(&a.state[u], ~kScLive) & kScLive)) return false;         // its other degree got there first
    publish(&a.colour[u], (int)u);
    return true;
  }
  if (OP == kScFwd) {
    if (s & kScF) return false;
    return !(atomicOr(&a.state[u], kScF) & kScF);
  }
  if (OP == kScBwd) {
    if (!(s & kScF)) return false;
    return (atomicAnd(&a.state[u], ~kScLive) & kScLive) != 0u;
  }
  if (OP == kScProp) {
    if (fresh(&a.colour[u]) <= c) return false;
    if (atomicMin(&a.colour[u], c) <= c) return false;
    return !(atomicOr(&a.state[u], qbit) & qbit);
  }
  // kScCollect
  if (fresh(&a.colour[u]) != c) return false;
  if (!(atomicAnd(&a.state[u], ~kScLive) & kScLive)) return false;
  atomicAdd(&a.din[c], 1);                               // the root's count of its component
  return true;
}

// up to N neighbours: the state loads, then the work, then the appends
template <int OP, int N>
__device__ __forceinline__ void sc_hit(const ScArgs& a, Index v, int c, unsigned qbit, const Index (&u)[N], bool (&ok)[N], WaveStage& o, int lane,
                                       unsigned& low) {
  unsigned s[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n;
    s[j] = ok[j] ? fresh(&a.state[u[j]]) : 0u;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) ok[j] = ok[j] && sc_apply<OP>(a, v, c, qbit, u[j], s[j]);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (OP == kScBwd && ok[j] && (unsigned)u[j] < low) low = (unsigned)u[j];
    stage_push<kScStage>(o, lane, ok[j], u[j]);
  }
}

// the list [b, e) of v walked by kThreads threads (t: this one's number among them); every lane of every wave of them calls it
template <int OP, int kThreads>
__device__ __forceinline__ void sc_walk(const ScArgs& a, const Index* __restrict__ ind, Index b, Index e, int t, int lane, Index v, int c,
                                        unsigned qbit, WaveStage& o, unsigned& low) {
  const QuadSpan s = quad_span(ind, b, e);
  const Index b4 = s.b4, nq = s.nq, te = s.te, nh = s.nh, ns = s.ns;
  if (kThreads == kWave || t < kWave) {
    Index u[1] = {0};
    bool ok[1] = {t < ns};
    if (ok[0]) u[0] = ind[t < nh ? b + t : te + (t - nh)];
    sc_hit<OP, 1>(a, v, c, qbit, u, ok, o, lane, low);
  }
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    bool ok[4];
    ok[0] = ok[1] = ok[2] = ok[3] = q < nq;
    const int4 w = ok[0] ? *reinterpret_cast<const int4*>(ind + b4 + 4 * (long long)q) : make_int4(0, 0, 0, 0);
    const Index u[4] = {w.x, w.y, w.z, w.w};
    sc_hit<OP, 4>(a, v, c, qbit, u, ok, o, lane, low);
  }
}

// one direction of one pass: the lists (ptr, ind) of the F vertices q[0 .. F) are walked.  Every thread of the grid calls it.
template <int OP>
__device__ __forceinline__ void sc_sweep(const ScArgs& a, const Index* __restrict__ ptr, const Index* __restrict__ ind, const Index* q,
                                         unsigned F, unsigned qclear, unsigned qbit, WaveStage& o, Index* s_big, int* s_nbig, unsigned& low) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const long long gwave = (long long)wave * gridDim.x + blockIdx.x, gwaves = (long long)gridDim.x * kPWaves;   // neighbouring chunks: different CUs
  const unsigned per = F >= (unsigned long long)gwaves * kWave ? (unsigned)kWave : (unsigned)((F + gwaves - 1) / gwaves);
  for (long long c0 = 0; c0 * per < F; c0 += gwaves) {
    if (tid == 0) *s_nbig = 0;
    __syncthreads();
    const long long i = (c0 + gwave) * per + lane;
    const bool have = lane < (int)per && i < (long long)F;
    Index v = 0, b = 0, e = 0;
    int c = 0;
    if (have) {
      v = fresh(&q[i]);
      if ((unsigned)v < (unsigned)a.n) {
        b = ptr[v];
        e = ptr[v + 1];
        if (OP == kScProp) atomicAnd(&a.state[v], ~qclear);                  // queued for this pass: no longer
        if (OP == kScProp || OP == kScCollect) c = fresh(&a.colour[v]);
      }
    }
    const Index len = e - b;
    if (len > kScWaveLen) s_big[atomicAdd(s_nbig, 1)] = v;                   // (at most one a thread: room for all)
    {                                                                        // the short lists, a lane each
      const bool mine = len <= kScLaneLen;
      const unsigned longest = wave_max_u32(mine && len > 0 ? (unsigned)len : 0u);
      for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
        Index u[4];
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ok[j] = mine && j0 + j < len;
          u[j] = ok[j] ? ind[b + j0 + j] : 0;
        }
        sc_hit<OP, 4>(a, v, c, qbit, u, ok, o, lane, low);
      }
    }
    unsigned long long mids = __ballot(len > kScLaneLen && len <= kScWaveLen);
    while (mids) {                                                           // the wave's lists, one after the other
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      sc_walk<OP, kWave>(a, ind, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, lane,
                         (Index)__builtin_amdgcn_readlane((int)v, l), __builtin_amdgcn_readlane(c, l), qbit, o, low);
    }
    __syncthreads();
    const int nbig = *s_nbig;
    for (int r = 0; r < nbig; ++r) {                                         // the workgroup's lists
      const Index w = s_big[r];
      const int cw = (OP == kScProp || OP == kScCollect) ? fresh(&a.colour[w]) : 0;
      sc_walk<OP, kPThreads>(a, ind, ptr[w], ptr[w + 1], tid, lane, w, cw, qbit, o, low);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPThreads) void scc_persistent_kernel(ScArgs a) {
  __shared__ Index s_stage[kPWaves][kScStage];
  __shared__ Index s_big[kPThreads];
  __shared__ int s_nbig;
  __shared__ unsigned long long s_red[kPWaves][3];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)gridDim.x * kPThreads;
  ScState* st = a.st;
  WaveStage o = {s_stage[wave], 0u, a.order, &st->slot[0].added, 0u, 0u};
  unsigned gen = 0;
  const long long n = a.n;
  const unsigned un = (unsigned)a.n;

  // every workgroup carries the same numbers: they come from the slots, read behind the barrier
  unsigned passes = 0, tail = 0, rm = 0, trimmed = 0, rounds = 0, comps = 0, largest = 0, trivial = 0;
  unsigned long long edges = 0;
  unsigned my_trivial = 0, my_largest = 0;               // this thread's part of the rounds' component sizes
  unsigned low = ~0u;                                    // ... and of the smallest member of the pivot's component
  ScSlot* sl = &st->slot[0];

  // a pass begins: its slot, the one after the next cleared, where it appends; and ends: the barrier, then what it appended
  auto pass_begin = [&](Index* buf, unsigned base) {
    sl = &st->slot[passes & 3u];
    o.counter = &sl->added;
    o.dst = buf;
    o.base = base;
    o.cap = un;
    if (blockIdx.x == 0 && tid == 0) {
      ScSlot* z = &st->slot[(passes + 2u) & 3u];
      publish(&z->added, 0u);
      publish(&z->inv_min, 0u);
      publish(&z->mx, 0ull);
      publish(&z->sum, 0ull);
    }
  };
  auto pass_end = [&](unsigned& added) -> bool {
    stage_flush(o, lane);
    if (!grid_sync(&st->bar, gen, false)) return false;
    added = fresh(&sl->added);
    ++passes;
    return true;
  };
  // the workgroup's part of a pass's sums, one atomic each
  auto reduce = [&](unsigned long long mx, unsigned inv, unsigned long long sum) {
    mx = wave_max_u64(mx);
    inv = wave_max_u32(inv);
    sum = wave_sum_u64(sum);
    if (lane == 0) { s_red[wave][0] = mx; s_red[wave][1] = inv; s_red[wave][2] = sum; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long bm = 0, bi = 0, bs = 0;
      for (int w = 0; w < kPWaves; ++w) { bm = s_red[w][0] > bm ? s_red[w][0] : bm; bi = s_red[w][1] > bi ? s_red[w][1] : bi; bs += s_red[w][2]; }
      if (bm) __hip_atomic_fetch_max(&sl->mx, bm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bi) __hip_atomic_fetch_max(&sl->inv_min, (unsigned)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bs) __hip_atomic_fetch_add(&sl->sum, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  // trimming to its fixpoint: order[rm, tail) lose their edges, what falls is appended
  auto trim = [&]() -> bool {
    while (rm < tail) {
      const unsigned end = tail;
      unsigned added;
      pass_begin(a.order, tail);
      sc_sweep<kScDecIn>(a, a.rptr, a.rind, a.order + rm, end - rm, 0u, 0u, o, s_big, &s_nbig, low);
      sc_sweep<kScDecOut>(a, a.cptr, a.cind, a.order + rm, end - rm, 0u, 0u, o, s_big, &s_nbig, low);
      if (!pass_end(added)) return false;
      rm = end;
      tail = tail + added > un ? un : tail + added;
      trimmed += added;
    }
    return true;
  };
  // a sweep that removes what it reaches, with order as its queue: order[from, tail) is its first frontier
  auto collect = [&](auto op, const Index* ptr, const Index* ind, unsigned from) -> bool {
    constexpr int OP = decltype(op)::value;
    while (from < tail) {
      const unsigned end = tail;
      unsigned added;
      pass_begin(a.order, tail);
      sc_sweep<OP>(a, ptr, ind, a.order + from, end - from, 0u, 0u, o, s_big, &s_nbig, low);
      if (OP == kScBwd) {
        const unsigned m = wave_min_u32(low);
        if (lane == 0 && m != ~0u) atomicMax(&st->giant_inv_min[0], ~m);
        low = ~0u;
      }
      if (!pass_end(added)) return false;
      from = end;
      tail = tail + added > un ? un : tail + added;
    }
    return true;
  };

  // ---- pass 0: the degrees; a vertex without an in- or an out-neighbour is a component
  {
    unsigned added;
    unsigned long long my_sum = 0;
    pass_begin(a.order, 0u);
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      const bool ok = v < n;
      bool dead = false;
      if (ok) {
        const int di = row_degree_no_diag(a.cptr, a.cind, (Index)v), dq = row_degree_no_diag(a.rptr, a.rind, (Index)v);
        dead = di == 0 || dq == 0;
        publish(&a.din[v], di);
        publish(&a.dout[v], dq);
        publish(&a.colour[v], (int)v);
        publish(&a.state[v], dead ? 0u : kScLive);
        my_sum += (unsigned long long)dq;
      }
      stage_push<kScStage>(o, lane, dead, (Index)v);
    }
    reduce(0ull, 0u, my_sum);
    if (!pass_end(added)) return;
    edges = fresh(&sl->sum);
    tail = added > un ? un : added;
    trimmed = tail;
  }
  if (!trim()) return;

  // ---- the giant component, forward-backward from the pivot
  if (tail < un) {
    unsigned added;
    unsigned long long best = 0;
    {                                                    // the largest din x dout
      unsigned long long my = 0;
      pass_begin(a.order, tail);
      for (long long v = gtid; v < n; v += gthreads)
        if (fresh(&a.state[v]) & kScLive) {
          const unsigned long long p = (unsigned long long)(unsigned)fresh(&a.din[v]) * (unsigned long long)(unsigned)fresh(&a.dout[v]);
          my = p > my ? p : my;
        }
      reduce(my, 0u, 0ull);
      if (!pass_end(added)) return;
      best = fresh(&sl->mx);
    }
    if (best != 0ull) {
      unsigned my = 0;                                   // the smallest vertex that has it
      pass_begin(a.order, tail);
      for (long long v = gtid; v < n; v += gthreads)
        if (fresh(&a.state[v]) & kScLive) {
          const unsigned long long p = (unsigned long long)(unsigned)fresh(&a.din[v]) * (unsigned long long)(unsigned)fresh(&a.dout[v]);
          if (p == best && ~(unsigned)v > my) my = ~(unsigned)v;
        }
      reduce(0ull, my, 0ull);
      if (!pass_end(added)) return;
      const unsigned pivot = ~fresh(&sl->inv_min);
      if (pivot < un) {
        // the pivot is removed and appended: the first frontier of both sweeps
        const unsigned from = tail;
        pass_begin(a.order, tail);
        if (blockIdx.x == 0 && wave == 0) {
          if (lane == 0) {
            publish(&a.state[pivot], kScF);
            atomicMax(&st->giant_inv_min[0], ~pivot);
          }
          stage_push<kScStage>(o, lane, lane == 0, (Index)pivot);
        }
        if (!pass_end(added)) return;
        tail = tail + added > un ? un : tail + added;
        // forward: F on what the pivot reaches; the frontiers alternate between qb and order's free end
        {
          const Index* fq = a.order + from;
          unsigned fF = tail - from;
          int side = 0;
          while (fF) {
            Index* ob = side == 0 ? a.qb : a.order;
            const unsigned obase = side == 0 ? 0u : tail;
            pass_begin(ob, obase);
            sc_sweep<kScFwd>(a, a.rptr, a.rind, fq, fF, 0u, 0u, o, s_big, &s_nbig, low);
            if (!pass_end(added)) return;
            fq = ob + obase;
            fF = added > un - obase ? un - obase : added;
            side ^= 1;
          }
        }
        // backward inside F: the component, removed as it is reached
        if (!collect(std::integral_constant<int, kScBwd>(), a.cptr, a.cind, from)) return;
        const unsigned label = ~fresh(&st->giant_inv_min[0]);
        for (long long i = (long long)from + gtid; i < (long long)tail; i += gthreads) {
          const Index v = fresh(&a.order[i]);
          if ((unsigned)v < un) publish(&a.colour[v], (int)label);
        }
        const unsigned size = tail - from;
        ++comps;
        largest = size;
        if (size == 1u) ++trivial;
        if (!trim()) return;
      }
    }
  }

  // ---- colouring rounds until nobody is live
  while (tail < un && rounds < un) {
    const bool even = (rounds & 1u) == 0u;
    const Index* pptr = even ? a.rptr : a.cptr;          // the colours travel along these lists
    const Index* pind = even ? a.rind : a.cind;
    const Index* qptr = even ? a.cptr : a.rptr;          // ... and the components are collected along these
    const Index* qind = even ? a.cind : a.rind;
    unsigned added;
    pass_begin(a.qb, 0u);                                // colour(v) = v, every live vertex queued
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      const bool live = v < n && (fresh(&a.state[v]) & kScLive);
      if (live) publish(&a.colour[v], (int)v);
      stage_push<kScStage>(o, lane, live, (Index)v);
    }
    if (!pass_end(added)) return;
    {
      const Index* fq = a.qb;
      unsigned fF = added > un ? un : added;
      int side = 1;
      unsigned par = 0;
      while (fF) {
        Index* ob = side == 0 ? a.qb : a.order;
        const unsigned obase = side == 0 ? 0u : tail;
        pass_begin(ob, obase);
        sc_sweep<kScProp>(a, pptr, pind, fq, fF, par ? kScQ0 : kScQ1, par ? kScQ1 : kScQ0, o, s_big, &s_nbig, low);
        if (!pass_end(added)) return;
        fq = ob + obase;
        fF = added > un - obase ? un - obase : added;
        side ^= 1;
        par ^= 1u;
      }
    }
    // the roots: colour(r) = r.  Removed and appended; din counts the component from here on
    const unsigned from = tail;
    pass_begin(a.order, tail);
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      bool root = false;
      if (v < n) {
        const unsigned s = fresh(&a.state[v]);
        root = (s & kScLive) && fresh(&a.colour[v]) == (int)v;
        if (root) {
          publish(&a.state[v], s & ~kScLive);
          publish(&a.din[v], 1);
        }
      }
      stage_push<kScStage>(o, lane, root, (Index)v);
    }
    if (!pass_end(added)) return;
    const unsigned nroots = added > un - tail ? un - tail : added;
    if (nroots == 0u) break;                             // (never: the smallest live vertex is a root)
    tail += nroots;
    comps += nroots;
    if (!collect(std::integral_constant<int, kScCollect>(), qptr, qind, from)) return;
    for (long long i = gtid; i < (long long)nroots; i += gthreads) {        // the sizes: final behind the last barrier
      const Index r = fresh(&a.order[from + i]);
      const unsigned size = (unsigned)r < un ? (unsigned)fresh(&a.din[r]) : 0u;
      if (size == 1u) ++my_trivial;
      my_largest = size > my_largest ? size : my_largest;
    }
    ++rounds;
    if (!trim()) return;
  }

  {
    unsigned added;
    pass_begin(a.order, tail);
    reduce((unsigned long long)my_largest, 0u, (unsigned long long)my_trivial);
    if (!pass_end(added)) return;
    const unsigned rl = (unsigned)fresh(&sl->mx);
    trivial += trimmed + (unsigned)fresh(&sl->sum);
    comps += trimmed;
    if (trimmed && largest < 1u) largest = 1u;
    if (rl > largest) largest = rl;
  }
  if (gtid == 0) {
    st->rec[0] = edges;
    st->rec[1] = comps;
    st->rec[2] = largest;
    st->rec[3] = trivial;
    st->rec[4] = trimmed;
    st->rec[5] = rounds;
    st->rec[6] = passes;
    st->rec[kScDone] = tail >= un ? 1ull : 2ull;         // 2: vertices left over (never)
  }
}

namespace {

grb_info scc_empty(grb_vector out, grb_scc_result* res) {                    // n = 0
  GRB_TRY(ctx_init());
  GRB_TRY(grb_vector_set_storage(out, GRB_DENSE));
  out->d_nnz = 0;
  grb_scc_result none = {};
  none.launches = 0;
  if (res) *res = none;
  return GRB_SUCCESS;
}

grb_info scc_run(grb_vector out, grb_matrix A, grb_scc_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  GRB_TRY(persistent_kernel_fits<scc_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, then six arrays of a word per vertex
  const size_t st_bytes = pad_bytes(sizeof(ScState));
  const size_t vw = pad_words((size_t)n);
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 24 * vw));
  ScArgs a;
  a.rptr = A->csr.ptr;
  a.rind = A->csr.ind;
  a.cptr = A->csc.ptr;
  a.cind = A->csc.ind;
  a.n = n;
  a.st = (ScState*)work.p;
  a.state = (unsigned*)((char*)work.p + st_bytes);
  a.din = (int*)(a.state + vw);
  a.dout = a.din + vw;
  a.colour = a.dout + vw;
  a.order = (Index*)(a.colour + vw);
  a.qb = a.order + vw;
  GRB_TRY(dense_out_prepare(out, n));                    // before anything runs; out stays as it was until the end

  GRB_TRY(bfs_lanes_fence(s));      // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
  hipLaunchKernelGGL(scc_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  unsigned long long h_rec[kScRec];
  GRB_HIP_TRY(hipMemcpyAsync(h_rec, a.st->rec, sizeof(h_rec), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // the call's one read
  if (h_rec[kScDone] != 1ull) return GRB_PANIC;          // a grid barrier gave up
  GRB_TRY(dense_out_commit(out, a.colour, n, s));
  grb_scc_result r = {};
  r.edges = (int64_t)h_rec[0];
  r.components = (int32_t)h_rec[1];
  r.largest = (int32_t)h_rec[2];
  r.trivial = (int32_t)h_rec[3];
  r.trimmed = (int32_t)h_rec[4];
  r.rounds = (int32_t)h_rec[5];
  r.passes = (int32_t)h_rec[6];
  r.launches = 1;
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_scc(grb_vector scc, grb_matrix A, grb_descriptor desc, grb_scc_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!scc || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || scc->nsize != n) return GRB_DIMENSION_MISMATCH;
  if (scc->dtype != GRB_I32 || (A->dtype != GRB_F32 && A->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (n == 0) return scc_empty(scc, result);
  if (!A->csr.ptr || A->csc_alias || !A->csc.ptr) return GRB_INVALID_OBJECT;   // a product result, the CSR-only format: no CSC of its own
  return scc_run(scc, A, result);
}
