// bcc.hip -- biconnected components, articulation points and bridges on the device: grb_bcc.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definition is this project's own:
//   a block is a class of "two edges lie on a common simple cycle, or are equal"; the blocks are numbered in ascending order
//   of their smallest edge key (min(u, v), max(u, v)); art(v) is the number of blocks that contain v.
//
// Tarjan-Vishkin on a BFS forest, and the whole loop is ONE co-resident launch (a 1024-thread workgroup per CU,
// persist_common.hpp's bounded grid barrier between its passes); the host reads one record when it is over.
//   comp     i32 per vertex: the smallest member of the vertex's connected component (minimum hooking + pointer jumping).
//   level    i32 per vertex: its BFS level; every vertex with comp(v) = v is a root and starts at level 0.
//   order    the ONE queue: every vertex in level order; lvoff: where a level begins in it.
//   parent   the smallest-numbered neighbour on the level above (atomicMin while the level is expanded).
//   size     vertices of the subtree: bottom-up by level, children add into their parent.
//   pre      a preorder number: top-down by level.  The roots take consecutive ranges of one counter, so pre is a permutation
//            of 0 .. n-1 and names the tree edge (parent(w), w) as slot pre(w); a child takes pre(parent) + 1 + what its
//            parent's cursor held, and adds its size to it.  Which sibling comes first is the atomics' order: EVERY preorder
//            gives the same blocks, and nothing that leaves the call depends on it (rounds and passes may).
//   low/high min / max of pre over the subtree's vertices and the other ends of their non-tree edges: a row walk, then
//            bottom-up by level with atomicMin / atomicMax into the parent.
//   lab      i32 per slot: the auxiliary graph's components by minimum hooking on pre + pointer jumping, to the fixpoint.
//            (i) a non-tree edge {v, w} joins pre(v) and pre(w) (a BFS tree's non-tree edge never joins an ancestor with a
//            descendant); (ii) the tree edge of w joins its parent's (v = parent(w), v not a root) when low(w) < pre(v) or
//            high(w) >= pre(v) + size(v).  A block's representative is its tree edge of smallest pre: a child of its top vertex.
//   outputs  the block of a tree edge is lab(pre(child)), of a non-tree edge lab(the larger pre of its ends).  Per
//            representative: the smallest CSR position among its entries above the diagonal (rows ascend: position order is
//            key order) and their number.  art(v) = [v is not a root] + its children that are representatives.
//   rows     of up to kBcLaneLen entries: a lane; up to kBcWaveLen: a wave, 16-byte index loads; longer: the workgroup.  The
//            vertices are dealt to the WAVES of the grid 64 at a time, neighbouring numbers to different waves.
// After the loop the representatives' (smallest position, slot) pairs are ordered by the library's radix sort: a block's
// number is its rank.  C is a count per row, the library's scan and one writing pass (a wave per row, in stored order).
// Working memory: 76 bytes per vertex and 2.5 KiB, one allocation; the sort brings 12 more per block of its own.  Nothing is
// proportional to the entries.
// Passes: 4 per BFS level (expansion, size, pre, low/high) + a hooking round's 1 + its jumps, for both hookings.  A path of a
// million vertices costs millions of barrier-bound passes: the known worst case, as a long path is in scc.hip.
#include "graph_common.hpp"

namespace grb {

constexpr int kBcLaneLen = 8;                            // a row of up to this many entries: one lane walks it
constexpr int kBcWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kBcStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kBcHops = 16;                              // labels a slot follows in one jumping pass
constexpr int kBcJumps = 40;                             // jumping passes a round, at most
constexpr int kBcRec = 16;
constexpr int kBcNone = 0x7fffffff;

struct BcSlot {                     // what one pass adds up; 128 bytes
  unsigned a, b;
  unsigned long long sum;
  unsigned pad[28];
};
struct BcState {                    // zeroed by the host before the launch
  GridBarrier bar;
  BcSlot slot[4];                   // pass p adds into slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned prebase[32];             // the roots' ranges of pre
  unsigned nrep[32];                // representatives listed
  unsigned largest[32];             // entries of the largest block
  unsigned flag[32];                // the symmetry check (graph_common.hpp): 1 = the CSR's and the CSC's structures differ
  unsigned long long rec[kBcRec];   // [0] off-diagonal entries [1] largest [2] blocks [3] bridges [4] articulation [5] components
                                    // [6] isolated [7] levels [8] rounds [9] passes [10] done
};
constexpr int kBcDone = 10;

struct BcArgs {
  const Index *ptr, *ind;
  Index n;
  int *comp, *level, *parent, *size, *pre, *low, *high, *cursor, *lab, *order, *lvoff, *minpos, *cnt, *art;
  unsigned long long* keys;         // the representatives: smallest position ...
  unsigned* pay;                    // ... and slot
  BcState* st;
};

// minimum hooking of the edge (x, y) in the label array L (L[i] <= i, always a member of i's component): the larger label's
// slot and the end that held it take the smaller label.  false: the two agree already
__device__ __forceinline__ bool bc_hook(int* L, int x, int y) {
  const int lx = fresh(&L[x]), ly = fresh(&L[y]);
  if (lx == ly) return false;
  const int lo = lx < ly ? lx : ly, hi = lx < ly ? ly : lx;
  atomicMin(&L[hi], lo);
  atomicMin(&L[lx < ly ? y : x], lo);
  return true;
}

// pre(v) as an index: inside 0 .. n-1 whatever the input holds
__device__ __forceinline__ int bc_pre(const BcArgs& a, Index v) {
  const int p = fresh(&a.pre[v]);
  return (unsigned)p < (unsigned)a.n ? p : 0;
}

struct BcLds {
  Index stage[kPWaves][kBcStage];   // a wave's staged appends
  Index big[kPThreads];             // the workgroup's rows of a deal
  int nbig;
  unsigned long long red[kPWaves][3];
};

// the row [b, e) of v walked by kThreads threads (t: this one's number among them); f.entry(v, position, column, valid) is
// called by every lane of a wave together
template <int kThreads, typename F>
__device__ __forceinline__ void bc_walk(const BcArgs& a, Index v, Index b, Index e, int t, F& f) {
  const QuadSpan s = quad_span(a.ind, b, e);
  const Index b4 = s.b4, nq = s.nq, te = s.te, nh = s.nh, ns = s.ns;
  if (kThreads == kWave || t < kWave) {
    const bool ok = t < ns;
    Index p = 0, u = 0;
    if (ok) {
      p = t < nh ? b + t : te + (t - nh);
      u = a.ind[p];
    }
    f.entry(v, p, u, ok);
  }
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    const bool ok = q < nq;
    const Index at = b4 + 4 * (ok ? q : 0);
    const int4 w = ok ? *reinterpret_cast<const int4*>(a.ind + at) : make_int4(0, 0, 0, 0);
    f.entry(v, at, w.x, ok);
    f.entry(v, at + 1, w.y, ok);
    f.entry(v, at + 2, w.z, ok);
    f.entry(v, at + 3, w.w, ok);
  }
}

// the rows of `count` vertices (list[first + i], or i itself without a list), dealt to the waves of the grid 64 at a time.
// F: wants(v), begin(v) (a row starts: once per lane for a lane's row, by every lane for a wave's or the workgroup's),
// entry(...), end(v, mine, shared) (shared: the lanes of the wave walked the same row)
template <typename F>
__device__ __forceinline__ void bc_rows(const BcArgs& a, BcLds& S, const int* list, long long first, long long count, F& f) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const long long gwave = (long long)wave * gridDim.x + blockIdx.x, gwaves = (long long)gridDim.x * kPWaves;
  for (long long base = 0; base < count; base += gwaves * kWave) {
    if (tid == 0) S.nbig = 0;
    __syncthreads();
    const long long i = base + (long long)lane * gwaves + gwave;             // neighbouring numbers: different waves and CUs (hubs come in runs)
    Index v = 0, b = 0, e = 0;
    if (i < count) {
      v = list ? (Index)fresh(&list[first + i]) : (Index)i;
      if ((unsigned)v < (unsigned)a.n && f.wants(v)) {
        b = a.ptr[v];
        e = a.ptr[v + 1];
      } else {
        v = 0;
      }
    }
    const Index len = e > b ? e - b : 0;
    if (len > kBcWaveLen) S.big[atomicAdd(&S.nbig, 1)] = v;                  // (at most one a thread: room for all)
    {                                                                        // the short rows, a lane each
      const bool mine = len > 0 && len <= kBcLaneLen;
      const unsigned longest = wave_max_u32(mine ? (unsigned)len : 0u);
      if (longest) {
        f.begin(v);
        for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
          Index u[4], p[4];
          bool ok[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ok[j] = mine && j0 + j < len;
            p[j] = ok[j] ? b + j0 + j : 0;
            u[j] = ok[j] ? a.ind[p[j]] : 0;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) f.entry(v, p[j], u[j], ok[j]);
        }
        f.end(v, mine, false);
      }
    }
    unsigned long long mids = __ballot(len > kBcLaneLen && len <= kBcWaveLen);
    while (mids) {                                                           // the wave's rows, one after the other
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
      f.begin(wv);
      bc_walk<kWave>(a, wv, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, f);
      f.end(wv, true, true);
    }
    __syncthreads();
    const int nbig = S.nbig;
    for (int r = 0; r < nbig; ++r) {                                         // the workgroup's rows
      const Index w = S.big[r];
      f.begin(w);
      bc_walk<kPThreads>(a, w, a.ptr[w], a.ptr[w + 1], tid, f);
      f.end(w, true, true);
    }
    __syncthreads();
  }
}

// ---- what the passes do with an entry ---------------------------------------------------------------------------------------
// the connected components: every off-diagonal entry hooks
struct BcCompHook {
  const BcArgs& a;
  unsigned changed;
  __device__ __forceinline__ bool wants(Index) const { return true; }
  __device__ __forceinline__ void begin(Index) {}
  __device__ __forceinline__ void entry(Index v, Index, Index u, bool ok) {
    if (ok && (unsigned)u < (unsigned)a.n && u != v && bc_hook(a.comp, v, u)) ++changed;
  }
  __device__ __forceinline__ void end(Index, bool, bool) {}
};

// a BFS level: the unseen neighbours join the queue (staged per wave in LDS, one reservation per batch), and every
// neighbour on the next level takes the smallest parent
struct BcExpand {
  const BcArgs& a;
  Index* stage;
  unsigned* tail;                   // appended in this level (a pass slot)
  unsigned base;                    // the queue's length before it
  int next;                         // the level being filled
  int lane;
  unsigned cnt;                     // staged: the same in every lane
  __device__ __forceinline__ bool wants(Index) const { return true; }
  __device__ __forceinline__ void begin(Index) {}
  __device__ __forceinline__ void flush() {
    if (cnt == 0u) return;
    __builtin_amdgcn_wave_barrier();
    unsigned at = 0;
    if (lane == 0) at = atomicAdd(tail, cnt);
    at = base + (unsigned)__shfl((int)at, 0, kWave);
    for (unsigned i = (unsigned)lane; i < cnt; i += kWave)
      if (at + i < (unsigned)a.n) publish(&a.order[at + i], (int)stage[i]);  // (always: a vertex joins once)
    __builtin_amdgcn_wave_barrier();
    cnt = 0u;
  }
  __device__ __forceinline__ void push(bool want, Index u) {
    const unsigned long long m = __ballot(want);
    if (m == 0ull) return;
    if (cnt + kWave > (unsigned)kBcStage) flush();
    if (want) stage[cnt + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = u;
    cnt += (unsigned)__popcll(m);
  }
  __device__ __forceinline__ void entry(Index v, Index, Index u, bool ok) {
    bool want = false;
    if (ok && (unsigned)u < (unsigned)a.n && u != v) {
      int lu = fresh(&a.level[u]);
      if (lu < 0) {
        lu = atomicCAS(&a.level[u], -1, next);
        if (lu < 0) { want = true; lu = next; }
      }
      if (lu == next && fresh(&a.parent[u]) > (int)v) atomicMin(&a.parent[u], (int)v);
    }
    push(want, u);
  }
  __device__ __forceinline__ void end(Index, bool, bool) {}
};

// is the entry (v, u) a non-tree edge?  pv = parent(v)
__device__ __forceinline__ bool bc_nontree(const BcArgs& a, Index v, int pv, Index u) {
  return (unsigned)u < (unsigned)a.n && u != v && (int)u != pv && fresh(&a.parent[u]) != (int)v;
}

// low / high of the vertex alone: pre over the other ends of its non-tree edges
struct BcLocal {
  const BcArgs& a;
  int lane;
  int pv;
  unsigned lo, hi1;                 // min of pre, max of pre + 1 (0: none)
  __device__ __forceinline__ bool wants(Index) const { return true; }
  __device__ __forceinline__ void begin(Index v) { pv = fresh(&a.parent[v]); lo = ~0u; hi1 = 0u; }
  __device__ __forceinline__ void entry(Index v, Index, Index u, bool ok) {
    if (ok && bc_nontree(a, v, pv, u)) {
      const unsigned x = (unsigned)bc_pre(a, u);
      lo = x < lo ? x : lo;
      hi1 = x + 1u > hi1 ? x + 1u : hi1;
    }
  }
  __device__ __forceinline__ void end(Index v, bool mine, bool shared) {
    if (shared) {
      lo = wave_min_u32(lo);
      hi1 = wave_max_u32(hi1);
      mine = lane == 0;
    }
    if (mine && hi1 != 0u) {
      if (fresh(&a.low[v]) > (int)lo) atomicMin(&a.low[v], (int)lo);
      if (fresh(&a.high[v]) < (int)(hi1 - 1u)) atomicMax(&a.high[v], (int)(hi1 - 1u));
    }
  }
};

// the auxiliary graph's rule (i): a non-tree edge joins the slots of its two ends
struct BcAuxHook {
  const BcArgs& a;
  int pv, xv;
  unsigned changed;
  __device__ __forceinline__ bool wants(Index v) const { return fresh(&a.level[v]) > 0; }
  __device__ __forceinline__ void begin(Index v) { pv = fresh(&a.parent[v]); xv = bc_pre(a, v); }
  __device__ __forceinline__ void entry(Index v, Index, Index u, bool ok) {
    if (ok && bc_nontree(a, v, pv, u) && bc_hook(a.lab, xv, bc_pre(a, u))) ++changed;
  }
  __device__ __forceinline__ void end(Index, bool, bool) {}
};

// the entries above the diagonal: their block's smallest position and their number.  A thread keeps the run of one
// representative and hands it over when the representative changes: a giant block is not an atomic per entry
struct BcCount {
  const BcArgs& a;
  int pv, xv;
  int rep;
  unsigned run;
  Index first;
  __device__ __forceinline__ bool wants(Index) const { return true; }
  __device__ __forceinline__ void begin(Index v) { pv = fresh(&a.parent[v]); xv = bc_pre(a, v); }
  __device__ __forceinline__ void flush() {
    if (run == 0u) return;
    atomicAdd((unsigned*)&a.cnt[rep], run);
    if (fresh(&a.minpos[rep]) > (int)first) atomicMin(&a.minpos[rep], (int)first);
    run = 0u;
  }
  __device__ __forceinline__ void entry(Index v, Index pos, Index u, bool ok) {
    if (!ok || (unsigned)u >= (unsigned)a.n || u <= v) return;
    int slot;
    if (fresh(&a.parent[u]) == (int)v) slot = bc_pre(a, u);
    else if ((int)u == pv) slot = xv;
    else { const int xu = bc_pre(a, u); slot = xu > xv ? xu : xv; }
    const int r = fresh(&a.lab[slot]);
    if (r != rep) { flush(); rep = r; first = pos; }
    first = pos < first ? pos : first;
    ++run;
  }
  __device__ __forceinline__ void end(Index, bool, bool) {}
};

__global__ __launch_bounds__(kPThreads) void bcc_persistent_kernel(BcArgs a) {
  __shared__ BcLds S;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  BcState* st = a.st;
  if (st->flag[0] != 0u) return;                         // not symmetric: every workgroup reads the same word
  const long long n = a.n;
  unsigned gen = 0, passes = 0, rounds = 0;
  BcSlot* sl = &st->slot[0];

  // a pass begins: its slot, the one after the next cleared; and ends: the barrier
  auto pass_begin = [&]() {
    sl = &st->slot[passes & 3u];
    if (blockIdx.x == 0 && tid == 0) {
      BcSlot* z = &st->slot[(passes + 2u) & 3u];
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
    if (lane == 0) { S.red[wave][0] = x; S.red[wave][1] = y; S.red[wave][2] = sum; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long bx = 0, by = 0, bs = 0;
      for (int w = 0; w < kPWaves; ++w) { bx += S.red[w][0]; by += S.red[w][1]; bs += S.red[w][2]; }
      if (bx) __hip_atomic_fetch_add(&sl->a, (unsigned)bx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (by) __hip_atomic_fetch_add(&sl->b, (unsigned)by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bs) __hip_atomic_fetch_add(&sl->sum, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  };
  // pointer jumping in L to the fixpoint: up to kBcHops labels a slot and pass.  false: a barrier gave up
  auto jump = [&](int* L) -> bool {
    for (int it = 0; it < kBcJumps; ++it) {
      unsigned open = 0;
      pass_begin();
      for (long long x = gtid; x < n; x += gthreads) {
        const int p0 = fresh(&L[x]);
        if (p0 == (int)x) continue;
        int p = p0;
        bool root = false;
        for (int hop = 0; hop < kBcHops && !root; ++hop) {                   // (a label only ever moves to a smaller member)
          const int pp = fresh(&L[p]);
          root = pp == p;
          p = pp;
        }
        if (p < p0) atomicMin(&L[x], p);
        if (!root) ++open;                                                   // not there yet: another pass
      }
      reduce(open, 0u, 0ull);
      if (!pass_end()) return false;
      if (fresh(&sl->a) == 0u) break;
    }
    return true;
  };

  // ---- pass 0: every vertex its own component and its own slot; the degrees
  unsigned long long offdiag = 0;
  unsigned isolated = 0;
  {
    unsigned my_iso = 0;
    unsigned long long my_sum = 0;
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const int d = row_degree_no_diag(a.ptr, a.ind, (Index)v);
      publish(&a.comp[v], (int)v);
      publish(&a.lab[v], (int)v);
      publish(&a.level[v], -1);
      publish(&a.parent[v], kBcNone);
      publish(&a.size[v], 1);
      publish(&a.pre[v], 0);
      publish(&a.low[v], 0);
      publish(&a.high[v], 0);
      publish(&a.cursor[v], 0);
      publish(&a.minpos[v], kBcNone);
      publish(&a.cnt[v], 0);
      publish(&a.art[v], 0);
      my_sum += (unsigned long long)d;
      if (d == 0) ++my_iso;
    }
    reduce(my_iso, 0u, my_sum);
    if (!pass_end()) return;
    isolated = fresh(&sl->a);
    offdiag = fresh(&sl->sum);
  }

  // ---- 1. the components: hooking rounds until no entry joins two labels (at most n + 1: the smallest label of a component
  //         reaches a neighbour more every round)
  for (long long r = 0; r <= n; ++r) {
    BcCompHook f = {a, 0u};
    pass_begin();
    bc_rows(a, S, nullptr, 0, n, f);
    reduce(f.changed, 0u, 0ull);
    if (!pass_end()) return;
    ++rounds;
    if (fresh(&sl->a) == 0u) break;
    if (!jump(a.comp)) return;
  }

  // ---- 2. the BFS forest: the roots, then a level a pass
  unsigned lo = 0, hi = 0;
  int levels = 0;
  {
    pass_begin();
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      const bool root = v < n && fresh(&a.comp[v]) == (int)v;
      const unsigned long long m = __ballot(root);
      if (m) {
        unsigned at = 0;
        if (lane == __ffsll((long long)m) - 1) at = atomicAdd(&sl->a, (unsigned)__popcll(m));
        at = (unsigned)__shfl((int)at, __ffsll((long long)m) - 1, kWave);
        if (root) {
          const unsigned slot = at + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
          publish(&a.level[v], 0);
          if (slot < (unsigned)n) publish(&a.order[slot], (int)v);
        }
      }
    }
    if (!pass_end()) return;
    hi = fresh(&sl->a);
    if (hi > (unsigned)n) hi = (unsigned)n;
    if (gtid == 0) { publish(&a.lvoff[0], 0); publish(&a.lvoff[1], (int)hi); }
  }
  const unsigned comps = hi;
  while (hi > lo && levels < (int)n) {                                       // (a level holds a vertex at least: at most n)
    ++levels;
    pass_begin();
    BcExpand f = {a, S.stage[wave], &sl->a, hi, levels, lane, 0u};
    bc_rows(a, S, a.order, (long long)lo, (long long)(hi - lo), f);
    f.flush();
    if (!pass_end()) return;
    unsigned top = hi + fresh(&sl->a);
    if (top > (unsigned)n) top = (unsigned)n;
    if (gtid == 0) publish(&a.lvoff[levels + 1], (int)top);
    lo = hi;
    hi = top;
  }
  // levels = the non-empty levels; level L is order[lvoff[L] .. lvoff[L + 1])

  // ---- 3. size, bottom-up
  for (int L = levels - 1; L >= 1; --L) {
    const long long s0 = fresh(&a.lvoff[L]), s1 = fresh(&a.lvoff[L + 1]);
    pass_begin();
    for (long long i = s0 + gtid; i < s1; i += gthreads) {
      const int w = fresh(&a.order[i]);
      atomicAdd(&a.size[fresh(&a.parent[w])], fresh(&a.size[w]));
    }
    if (!pass_end()) return;
  }
  // ---- 4. pre, top-down: the roots' ranges, then a child behind its earlier siblings
  if (levels > 0) {
    const long long s1 = fresh(&a.lvoff[1]);
    pass_begin();
    for (long long i = gtid; i < s1; i += gthreads) {
      const int w = fresh(&a.order[i]);
      const int x = (int)atomicAdd(&st->prebase[0], (unsigned)fresh(&a.size[w]));
      publish(&a.pre[w], x);
      publish(&a.low[w], x);
      publish(&a.high[w], x);
    }
    if (!pass_end()) return;
  }
  for (int L = 1; L < levels; ++L) {
    const long long s0 = fresh(&a.lvoff[L]), s1 = fresh(&a.lvoff[L + 1]);
    pass_begin();
    for (long long i = s0 + gtid; i < s1; i += gthreads) {
      const int w = fresh(&a.order[i]);
      const int p = fresh(&a.parent[w]);
      const int x = fresh(&a.pre[p]) + 1 + atomicAdd(&a.cursor[p], fresh(&a.size[w]));
      publish(&a.pre[w], x);
      publish(&a.low[w], x);
      publish(&a.high[w], x);
    }
    if (!pass_end()) return;
  }
  // ---- 5. low / high: the vertex's own non-tree edges, then bottom-up
  {
    BcLocal f = {a, lane, 0, ~0u, 0u};
    pass_begin();
    bc_rows(a, S, nullptr, 0, n, f);
    if (!pass_end()) return;
  }
  for (int L = levels - 1; L >= 1; --L) {
    const long long s0 = fresh(&a.lvoff[L]), s1 = fresh(&a.lvoff[L + 1]);
    pass_begin();
    for (long long i = s0 + gtid; i < s1; i += gthreads) {
      const int w = fresh(&a.order[i]);
      const int p = fresh(&a.parent[w]);
      const int lw = fresh(&a.low[w]), hw = fresh(&a.high[w]);
      if (fresh(&a.low[p]) > lw) atomicMin(&a.low[p], lw);
      if (fresh(&a.high[p]) < hw) atomicMax(&a.high[p], hw);
    }
    if (!pass_end()) return;
  }
  // ---- 6. the auxiliary graph's components
  for (long long r = 0; r <= n; ++r) {
    BcAuxHook f = {a, 0, 0, 0u};
    pass_begin();
    for (long long w = gtid; w < n; w += gthreads) {                         // rule (ii)
      if (fresh(&a.level[w]) <= 0) continue;
      const int v = fresh(&a.parent[w]);
      if (fresh(&a.level[v]) <= 0) continue;
      const int xv = bc_pre(a, v);
      if ((fresh(&a.low[w]) < xv || fresh(&a.high[w]) >= xv + fresh(&a.size[v])) && bc_hook(a.lab, bc_pre(a, (Index)w), xv)) ++f.changed;
    }
    bc_rows(a, S, nullptr, 0, n, f);                                         // rule (i)
    reduce(f.changed, 0u, 0ull);
    if (!pass_end()) return;
    ++rounds;
    if (fresh(&sl->a) == 0u) break;
    if (!jump(a.lab)) return;
  }
  // ---- 7. per representative: smallest position and entries; art's children
  {
    BcCount f = {a, 0, 0, -1, 0u, 0};
    pass_begin();
    bc_rows(a, S, nullptr, 0, n, f);
    f.flush();
    for (long long base = 0; base < n; base += gthreads) {
      const long long w = base + gtid;
      bool is = false;
      int p = 0;
      if (w < n && fresh(&a.level[w]) > 0) {
        const int x = bc_pre(a, (Index)w);
        is = fresh(&a.lab[x]) == x;
        p = fresh(&a.parent[w]);
      }
      const unsigned long long m = __ballot(is);
      if (m == 0ull) continue;
      const int l0 = __ffsll((long long)m) - 1;
      const int p0 = __shfl(p, l0, kWave);
      if (__ballot(is && p != p0) == 0ull) {                                 // one parent (a star's leaves): one atomic
        if (lane == l0) atomicAdd(&a.art[p0], __popcll(m));
      } else if (is) {
        atomicAdd(&a.art[p], 1);
      }
    }
    if (!pass_end()) return;
  }
  unsigned blocks = 0, bridges = 0, artic = 0;
  {
    unsigned my_blocks = 0, my_bridges = 0, my_largest = 0;
    unsigned long long my_art = 0;
    pass_begin();
    for (long long base = 0; base < n; base += gthreads) {
      const long long x = base + gtid;
      unsigned mp = (unsigned)kBcNone;
      if (x < n) {
        mp = (unsigned)fresh(&a.minpos[x]);
        const int t = fresh(&a.art[x]) + (fresh(&a.level[x]) > 0 ? 1 : 0);
        a.art[x] = t;                                                        // (read by the host's copy alone)
        if (t >= 2) ++my_art;
      }
      const bool is = mp != (unsigned)kBcNone;
      if (is) {
        const unsigned c = (unsigned)fresh(&a.cnt[x]);
        ++my_blocks;
        if (c == 1u) ++my_bridges;
        my_largest = c > my_largest ? c : my_largest;
      }
      const unsigned long long m = __ballot(is);
      if (m) {
        const int l0 = __ffsll((long long)m) - 1;
        unsigned at = 0;
        if (lane == l0) at = atomicAdd(&st->nrep[0], (unsigned)__popcll(m));
        at = (unsigned)__shfl((int)at, l0, kWave) + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (is && at < (unsigned)n) {
          a.keys[at] = (unsigned long long)mp;
          a.pay[at] = (unsigned)x;
        }
      }
    }
    my_largest = wave_max_u32(my_largest);
    if (lane == 0 && my_largest) atomicMax(&st->largest[0], my_largest);
    reduce(my_blocks, my_bridges, my_art);
    if (!pass_end()) return;
    blocks = fresh(&sl->a);
    bridges = fresh(&sl->b);
    artic = (unsigned)fresh(&sl->sum);
  }
  if (gtid == 0) {
    st->rec[0] = offdiag;
    st->rec[1] = fresh(&st->largest[0]);
    st->rec[2] = blocks;
    st->rec[3] = bridges;
    st->rec[4] = artic;
    st->rec[5] = comps;
    st->rec[6] = isolated;
    st->rec[7] = (unsigned long long)levels;
    st->rec[8] = rounds;
    st->rec[9] = passes;
    st->rec[kBcDone] = 1ull;
  }
}

// ---- after the loop ---------------------------------------------------------------------------------------------------------
// a block's number is its representative's rank by smallest position
__global__ __launch_bounds__(kBlock) void bc_number_kernel(const unsigned* __restrict__ pay, long long B, Index n, int* __restrict__ number) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < B; i += (long long)gridDim.x * kBlock)
    if (pay[i] < (unsigned)n) number[pay[i]] = (int)i;
}

// the entry (v, u), u != v: its block's slot
__device__ __forceinline__ int bc_entry_rep(const BcArgs& a, Index v, Index u) {
  int slot;
  const int xv = a.pre[v], xu = a.pre[u];
  if (a.parent[u] == (int)v) slot = xu;
  else if (a.parent[v] == (int)u) slot = xv;
  else slot = xu > xv ? xu : xv;
  if ((unsigned)slot >= (unsigned)a.n) slot = 0;
  const int r = a.lab[slot];
  return (unsigned)r < (unsigned)a.n ? r : 0;
}
__device__ __forceinline__ bool bc_keep(const BcArgs& a, Index v, Index u, int bridges_only, int* rep) {
  if ((unsigned)u >= (unsigned)a.n || u == v) return false;
  *rep = bc_entry_rep(a, v, u);
  return !bridges_only || a.cnt[*rep] == 1;
}

// a wave per row.  kWrite = false: the entries C keeps of the row; true: they are written in stored order behind optr[row]
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void bc_rows_kernel(BcArgs a, int bridges_only, const int* __restrict__ number, unsigned* __restrict__ counts,
                                                         const unsigned* __restrict__ optr, Index* __restrict__ oind, int* __restrict__ oval) {
  const int lane = lane_id();
  const long long waves = (long long)gridDim.x * kWavesPerBlock;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < a.n; v += waves) {
    const Index b = a.ptr[v], e = a.ptr[v + 1];
    unsigned at = kWrite ? optr[v] : 0u;
    for (Index j0 = b; j0 < e; j0 += kWave) {
      const Index j = j0 + lane;
      int rep = 0;
      Index u = 0;
      bool keep = false;
      if (j < e) {
        u = a.ind[j];
        keep = bc_keep(a, (Index)v, u, bridges_only, &rep);
      }
      const unsigned long long m = __ballot(keep);
      if (kWrite && keep) {
        const unsigned o = at + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        oind[o] = u;
        oval[o] = number[rep];
      }
      at += (unsigned)__popcll(m);
    }
    if (!kWrite && lane == 0) counts[v] = at;
  }
}

namespace {

grb_info bcc_run(grb_matrix C, grb_vector art, grb_matrix A, int mode, grb_bcc_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  const bool both = C && C->format != 1;
  grb_bcc_result r = {};
  Side sr, sc;
  if (n > 0) GRB_TRY(persistent_kernel_fits<bcc_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, sixteen words per vertex (lvoff has n + 2), the representatives' pairs, the scan's totals
  const size_t st_bytes = pad_bytes(sizeof(BcState));
  const size_t vw = pad_words((size_t)n + 2);
  const size_t scan_bytes = (device_scan_u32_scratch((long long)n + 1) + 63) & ~(size_t)63;   // (the last array: to 64 bytes)
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 76 * vw + scan_bytes + 64));
  BcArgs a;
  a.ptr = A->csr.ptr;
  a.ind = A->csr.ind;
  a.n = n;
  a.st = (BcState*)work.p;
  a.keys = (unsigned long long*)((char*)work.p + st_bytes);
  a.pay = (unsigned*)(a.keys + vw);
  a.comp = (int*)(a.pay + vw);
  a.level = a.comp + vw;
  a.parent = a.level + vw;
  a.size = a.parent + vw;
  a.pre = a.size + vw;
  a.low = a.pre + vw;
  a.high = a.low + vw;
  a.cursor = a.high + vw;
  a.lab = a.cursor + vw;
  a.order = a.lab + vw;
  a.lvoff = a.order + vw;
  a.minpos = a.lvoff + vw;
  a.cnt = a.minpos + vw;
  a.art = a.cnt + vw;
  int* d_number = a.art + vw;                            // a representative's block number
  unsigned* d_counts = (unsigned*)(d_number + vw);       // C's entries per row, then its pointers
  unsigned* d_scan = d_counts + vw;
  if (art) GRB_TRY(dense_out_prepare(art, n));           // before anything runs; art stays as it was until the end
  long long B = 0, m = 0;
  if (n > 0) {
    GRB_TRY(bfs_lanes_fence(s));    // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
    GRB_HIP_TRY(hipEventRecord(ev.a, s));
    GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
    launch_symmetry_check<false>(A, &a.st->flag[0], s);  // (the values are never read)
    hipLaunchKernelGGL(bcc_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
    GRB_HIP_TRY(hipGetLastError());
    struct { unsigned flag[32]; unsigned long long rec[kBcRec]; } h;
    GRB_HIP_TRY(hipMemcpyAsync(&h, a.st->flag, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // the call's one read of the loop
    if (h.flag[0] != 0u) return GRB_INVALID_VALUE;       // A's CSR and CSC differ: not symmetric
    if (h.rec[kBcDone] != 1ull) return GRB_PANIC;        // a grid barrier gave up
    B = (long long)h.rec[2];
    if (B > (long long)n) B = (long long)n;
    r.edges = (int64_t)(h.rec[0] / 2);
    r.largest = (int64_t)h.rec[1];
    r.blocks = (int32_t)h.rec[2];
    r.bridges = (int32_t)h.rec[3];
    r.articulation = (int32_t)h.rec[4];
    r.components = (int32_t)h.rec[5];
    r.isolated = (int32_t)h.rec[6];
    r.levels = (int32_t)h.rec[7];
    r.rounds = (int32_t)h.rec[8];
    r.passes = (int32_t)h.rec[9];
    r.launches = 1;
  }
  // ---- C's arrays: the blocks' numbers, a count per row, the scan, one writing pass
  if (C) {
    if (n > 0) {
      GRB_TRY(device_sort_pairs(a.keys, a.pay, B, key_bits((long long)A->nvals + 1), 0));
      if (B > 0) hipLaunchKernelGGL(bc_number_kernel, dim3(stream_grid(B)), dim3(kBlock), 0, s, a.pay, B, n, d_number);
      GRB_HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * ((size_t)n + 1), s));
      hipLaunchKernelGGL(bc_rows_kernel<false>, dim3(stream_grid((long long)n * kWave)), dim3(kBlock), 0, s, a, mode, d_number, d_counts,
                         (const unsigned*)nullptr, (Index*)nullptr, (int*)nullptr);
      GRB_HIP_TRY(hipGetLastError());
      GRB_TRY(device_exclusive_scan_u32_in(d_counts, (long long)n + 1, d_scan));
      unsigned total = 0;
      GRB_HIP_TRY(hipMemcpy(&total, d_counts + n, 4, hipMemcpyDeviceToHost));
      m = (long long)total;
    }
    GRB_TRY(side_alloc(&sr, n, m));
    if (both) GRB_TRY(side_alloc(&sc, n, m));
    if (n > 0) {
      GRB_HIP_TRY(hipMemcpyAsync(sr.ptr.p, d_counts, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
      if (m > 0) {
        hipLaunchKernelGGL(bc_rows_kernel<true>, dim3(stream_grid((long long)n * kWave)), dim3(kBlock), 0, s, a, mode, d_number, (unsigned*)nullptr,
                           d_counts, (Index*)sr.ind.p, (int*)sr.val.p);
        GRB_HIP_TRY(hipGetLastError());
      }
      GRB_HIP_TRY(hipMemcpyAsync(sr.h_ptr.data(), sr.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
      if (both) GRB_TRY(side_mirror(&sc, sr, n, m, s));  // the structure is symmetric and an edge has one block: the CSC is a copy
    } else {
      GRB_HIP_TRY(hipMemsetAsync(sr.ptr.p, 0, 4, s));
      if (both) GRB_HIP_TRY(hipMemsetAsync(sc.ptr.p, 0, 4, s));
    }
  }
  if (n > 0) {
    GRB_HIP_TRY(hipEventRecord(ev.b, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
    GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  } else {
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  if (C && both) sc.h_ptr = sr.h_ptr;
  // everything that can fail is behind us, but the CSC's plan (attach builds it before it touches C) and a copy.  A, which
  // may be C, has been read for the last time
  if (C) GRB_TRY(attach(C, &sr, both ? &sc : nullptr));
  if (art) GRB_TRY(dense_out_commit(art, a.art, n, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_bcc(grb_matrix C, grb_vector art, grb_matrix A, int mode, grb_descriptor desc, grb_bcc_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || (C && (C->nrows != n || C->ncols != n)) || (art && art->nsize != n)) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || (art && art->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (C && C->dtype != GRB_I32) return GRB_DOMAIN_MISMATCH;
  if (mode != GRB_BCC_BLOCKS && mode != GRB_BCC_BRIDGES) return GRB_INVALID_VALUE;
  if (n > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return bcc_run(C, art, A, mode, result);
}
