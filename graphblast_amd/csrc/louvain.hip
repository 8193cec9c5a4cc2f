// louvain.hip -- Louvain community detection on the device: grb_louvain.  The contract, the rule and why every accepted round
// strictly increases the modularity are the comment in include/grb_hip.h and DESIGN.md 5.4s; the reference has no such driver
// (graphblas/algorithm/), the definition is this project's own.  Everything that decides anything is a 64-bit integer:
//   QN = W * sum_x in(x) - sum_x tot(x)^2,   score(v, x) = W * e(v, x) - k(v) * tot(x),   gain = score - stay.
//
// Setup, plain launches: the weights checked and turned into i32 once (lv_weights_kernel, W by graph_common.hpp's fixed-shape
// integer sum), and per level k, c = identity, tot = k and the longest row (lv_init_kernel).
// A level is ONE co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid barrier between its
// passes); the host reads one record per level.  A round:
//   P   propose.  Every vertex with a stored row folds it by the neighbour's community and keeps the best score, the
//       smallest community on a tie.  Rows are dealt by length, as in cdlp.hip:
//         up to kLvLaneLen entries    a lane, all pairs compared in registers
//         up to kLvWaveLen            a wave, an entry a lane, all pairs compared by lane broadcasts
//         up to kLvSmallLen           a wave with its own LDS table of (community, 32-bit weight sum) pairs: e <= W < 2^31
//         up to kLvBlockLen           the workgroup with the whole LDS table (the waves' tables are its slices)
//         longer                      queued; after one more barrier a workgroup folds it into a global array of n words of
//                                     its own (communities are < n), reads the sums back and puts the zeros back
//       From the wave's table on, rows are streamed as 16-byte quads, indices and weights together (quad_span).
//       A proposer (v -> d, g) adds k(v) to K(d) and raises best(c(v)) and best(d) to g: 64-bit integer atomicMax.
//   C   claim.  Every proposer whose g is the maximum of a community it touches lowers win of that community to v: a 32-bit
//       atomicMin among the holders of the maximum, msf.hip's two-step key ((g, v) does not fit one 64-bit atomic).
//   A   accept.  win(c(v)) = v, and win(d) = v or (win(d) proposes to enter d, and g > k(v) * (K(d) - k(v))).
//   U   apply and clear.  c(v) = d, tot by integer atomics; best, win and K of what the round touched go back to their
//       identities.  No floating-point atomics anywhere, nothing is allocated inside a level.
// The level's last pass sums in(x) and tot(x)^2 for the record.  Between levels: grb_relabel on c in place, then
// grb_contract(PLUS, loops = 1) into a CSR-only i32 matrix -- the existing entries, no second sort path.
// Working memory: 44 bytes per vertex and 4 per stored entry of A (the i32 weights), the composed assignment (8 bytes per
// vertex), and for n > kLvBlockLen the count arrays for the long rows: as many as fit in kLvPoolBytes, one a CU at most, at
// least one (alone above kLvPoolBytes where n is above 32 M); allocated and zeroed once a call, long row or not.
// Nobody has measured any constant here: they mirror cdlp.hip's and matching.hip's until a measurement says otherwise.
#include <climits>
#include <memory>

#include "graph_common.hpp"

namespace grb {

constexpr int kLvLaneLen = 8;                            // a row of up to this many entries: one lane
constexpr int kLvWaveLen = 64;                           // ... a wave, all pairs
constexpr int kLvSmallLen = 256;                         // ... a wave with its slice of the LDS table
constexpr int kLvSmallBits = 8;                          // the slice: 256 pairs, 2 KiB, full at most (distinct keys <= entries)
constexpr int kLvBlockLen = 2048;                        // ... the workgroup with the whole table; longer: a global array
constexpr int kLvBlockBits = 12;                         // the table: 4096 pairs, 32 KiB, at most half full
constexpr int kLvSlots = 1 << kLvBlockBits;
constexpr size_t kLvPoolBytes = (size_t)128 << 20;       // the long rows' count arrays together, at most (cdlp.hip's figure)
constexpr unsigned kLvEmpty = 0xffffffffu;
constexpr int kLvNoWin = INT_MAX;
constexpr int kLvSumBlocks = 256;                        // partial sums of W, at most
constexpr int kLvRec = 8;
static_assert((kPWaves << kLvSmallBits) == kLvSlots, "the waves' tables are the slices of the workgroup's");

struct LvSlot {                     // what one pass adds up; 128 bytes
  unsigned a, b;
  unsigned long long sum, sum2;
  unsigned pad[26];
};
struct LvState {                    // zeroed by the host before the launch
  GridBarrier bar;
  LvSlot slot[4];                   // pass p adds into slot[p & 3]; workgroup 0 clears slot[(p + 2) & 3] meanwhile
  unsigned maxlen[32];              // the longest row (lv_init_kernel)
  unsigned long long rec[kLvRec];   // [0] rounds [1] moves [2] proposals [3] passes [4] sum in(x) [5] sum tot(x)^2 [6] done
};
constexpr int kLvDone = 6;

struct LvArgs {
  const Index *ptr, *ind;
  const int* val;                   // the i32 weights, aligned like ind
  Index n;
  long long nnz, W;
  int max_rounds;
  Index* c;                         // the community
  const unsigned* k;                // the row sum with the diagonal
  unsigned* tot;
  Index* prop_d;                    // the proposal's destination, or -1
  unsigned long long* prop_g;       // ... and its gain; 0 once rejected
  unsigned long long* best;         // per community: the largest gain that claims it
  int* win;                         // ... and the smallest vertex that holds it
  unsigned* K;                      // ... and the k of everybody who proposes to enter it (<= W: 32 bits)
  Index* longlist;
  unsigned* pool;                   // pool_count arrays of pool_stride words, all zero between rows
  size_t pool_stride;
  int pool_count;
  LvState* st;
};

// ---- setup -------------------------------------------------------------------------------------------------------------------
// w[p] = the weight of stored entry p as an i32 (1 when the values are not read); flag |= 1 for a bad one; the blocks' sums
__global__ __launch_bounds__(kBlock) void lv_weights_kernel(const unsigned* __restrict__ val, long long nnz, int weighted, int f32, int* __restrict__ w,
                                                            unsigned* __restrict__ flag, unsigned long long* __restrict__ partial) {
  long long is = 0;
  bool bad = false;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += (long long)gridDim.x * kBlock) {
    int x = 1;
    if (weighted) {
      const unsigned b = weight_canon(val[p], f32);
      if (f32) {
        const float f = __uint_as_float(b);
        const bool ok = f >= 0.f && f <= 16777216.f && f == truncf(f);       // (a NaN fails the first)
        bad |= !ok;
        x = ok ? (int)f : 0;
      } else {
        bad |= (int)b < 0;
        x = (int)b < 0 ? 0 : (int)b;
      }
    }
    w[p] = x;
    is += x;
  }
  if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(flag, 1u);
  weight_block_sum<false>(0.0, is, partial);
}

// a wave a vertex: k = the row's sum, c = v, tot = k, the claim arrays at their identities; the longest row
__global__ __launch_bounds__(kBlock) void lv_init_kernel(LvArgs a, unsigned* __restrict__ k) {
  const int lane = lane_id();
  const long long gwaves = (long long)gridDim.x * kWavesPerBlock;
  unsigned longest = 0;
  for (long long v = (long long)blockIdx.x * kWavesPerBlock + wave_id(); v < a.n; v += gwaves) {
    const Index b = a.ptr[v], e = a.ptr[v + 1];
    unsigned s = 0;
    for (Index p = b + lane; p < e; p += kWave) s += (unsigned)a.val[p];
    s = wave_sum_u32(s);
    if (e > b && (unsigned)(e - b) > longest) longest = (unsigned)(e - b);
    if (lane == 0) {
      k[v] = s;
      a.c[v] = (Index)v;
      a.tot[v] = s;
      a.prop_d[v] = -1;
      a.prop_g[v] = 0ull;
      a.best[v] = 0ull;
      a.win[v] = kLvNoWin;
      a.K[v] = 0u;
    }
  }
  if (lane == 0 && longest) atomicMax(&a.st->maxlen[0], longest);
}

// ---- the propose pass ----------------------------------------------------------------------------------------------------------
constexpr long long kLvNone = LLONG_MIN;                 // no candidate yet

// v's best score bs at community bx (bx < 0: none): the proposal, its claims.  Returns 1 when v proposes.
__device__ __forceinline__ unsigned lv_settle(const LvArgs& a, Index v, Index ca, unsigned kv, unsigned ea, long long bs, Index bx) {
  if (bx >= 0) {
    const long long ta = (long long)fresh(&a.tot[ca]);
    const long long stay = a.W * (long long)ea - (long long)kv * (ta - (long long)kv);
    const long long g = bs - stay;
    if (g > 0) {
      publish(&a.prop_g[v], (unsigned long long)g);
      publish(&a.prop_d[v], bx);
      atomicMax(&a.best[ca], (unsigned long long)g);
      atomicMax(&a.best[bx], (unsigned long long)g);
      atomicAdd(&a.K[bx], kv);
      return 1u;
    }
  }
  publish(&a.prop_d[v], (Index)-1);
  return 0u;
}

// (s, x) replaces (bs, bx) when it is the larger score, or the same at the smaller community
__device__ __forceinline__ void lv_better(long long s, unsigned x, long long& bs, unsigned& bx) {
  if (s > bs || (s == bs && x < bx)) { bs = s; bx = x; }
}

// the (community, weight sum) table: a slot is claimed by a compare-and-swap of its key; it has room for every distinct key
template <int kBits>
__device__ __forceinline__ void lv_insert(unsigned* key, unsigned* sum, unsigned x, unsigned w) {
  unsigned h = (x * 0x9e3779b1u) >> (32 - kBits);
  for (;;) {
    const unsigned prev = atomicCAS(&key[h], kLvEmpty, x);
    if (prev == kLvEmpty || prev == x) break;
    h = (h + 1u) & ((1u << kBits) - 1u);
  }
  if (w) atomicAdd(&sum[h], w);
}

// f(community of the other end, weight) for every off-diagonal entry of v's row [b, e), thread t of kThreads: the entries in
// front of and behind the 16-byte quads one a thread, then a quad of indices and a quad of weights a thread and step, the
// four communities gathered before the first f
template <int kThreads, typename F>
__device__ __forceinline__ void lv_walk(const LvArgs& a, Index v, Index b, Index e, int t, F f) {
  const QuadSpan s = quad_span(a.ind, b, e);
  if (t < s.ns) {
    const Index p = t < s.nh ? b + t : s.te + (t - s.nh);
    const Index u = a.ind[p];
    if (u != v && (unsigned)u < (unsigned)a.n) f((unsigned)fresh(&a.c[u]), (unsigned)a.val[p]);
  }
  for (Index q = t; q < s.nq; q += kThreads) {
    const Index at = s.b4 + 4 * q;
    const int4 iu = *reinterpret_cast<const int4*>(a.ind + at);
    const int4 iw = *reinterpret_cast<const int4*>(a.val + at);
    const Index u[4] = {iu.x, iu.y, iu.z, iu.w};
    const int w[4] = {iw.x, iw.y, iw.z, iw.w};
    bool ok[4];
    unsigned cu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ok[j] = u[j] != v && (unsigned)u[j] < (unsigned)a.n;
      cu[j] = ok[j] ? (unsigned)fresh(&a.c[u[j]]) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) f(cu[j], (unsigned)w[j]);
  }
}

struct LvLds {
  Index big[kPThreads];             // the batch's rows for the workgroup
  int nbig;
  long long bs[kPWaves];
  unsigned bx[kPWaves], ea[kPWaves];
};

// this thread's slots of a table: the own community's sum, the best score among the others; the slots are emptied
template <int kSlotsHere, int kThreads>
__device__ __forceinline__ void lv_table_scan(const LvArgs& a, unsigned* key, unsigned* sum, int t, unsigned ca, unsigned kv, unsigned& ea, long long& bs,
                                              unsigned& bx) {
  constexpr int kPer = kSlotsHere / kThreads;
  unsigned x[kPer], e[kPer], tt[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    x[j] = key[t + j * kThreads];
    e[j] = sum[t + j * kThreads];
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) tt[j] = x[j] != kLvEmpty && x[j] != ca ? fresh(&a.tot[x[j]]) : 0u;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (x[j] == kLvEmpty) continue;
    key[t + j * kThreads] = kLvEmpty;
    sum[t + j * kThreads] = 0u;
    if (x[j] == ca) ea = e[j];
    else lv_better(a.W * (long long)e[j] - (long long)kv * (long long)tt[j], x[j], bs, bx);
  }
}

// the wave's best of its lanes' (bs, bx), in every lane
__device__ __forceinline__ void lv_wave_best(long long& bs, unsigned& bx) {
  const long long mx = wave_reduce(bs, [](long long x, long long y) { return x > y ? x : y; });
  bx = wave_min_u32(bs == mx ? bx : kLvEmpty);
  bs = mx;
}
// ... and the workgroup's, in thread 0 (ea: the waves' sums added); every thread calls it
__device__ __forceinline__ void lv_block_best(LvLds& L, int tid, int lane, int wave, long long& bs, unsigned& bx, unsigned& ea) {
  lv_wave_best(bs, bx);
  ea = wave_sum_u32(ea);
  if (lane == 0) { L.bs[wave] = bs; L.bx[wave] = bx; L.ea[wave] = ea; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kPWaves; ++w) {
      lv_better(L.bs[w], L.bx[w], bs, bx);
      ea += L.ea[w];
    }
  }
}

// the short and the middle rows of the level, by their length classes; long rows are queued.  The whole grid calls it together.
__device__ __forceinline__ unsigned lv_propose(const LvArgs& a, LvSlot* sl, unsigned* s_key, unsigned* s_sum, LvLds& L, int tid, int lane, int wave,
                                               long long gwave, long long gwaves) {
  unsigned props = 0;
  const long long n = a.n;
  unsigned* const wkey = s_key + (wave << kLvSmallBits);
  unsigned* const wsum = s_sum + (wave << kLvSmallBits);
  for (long long base = 0; base < n; base += gwaves * kWave) {
    if (tid == 0) L.nbig = 0;
    __syncthreads();
    const long long i = base + (long long)lane * gwaves + gwave;             // neighbouring vertices: different waves and CUs (hubs come in runs)
    Index v = 0, b = 0, e = 0;
    if (i < n) {
      v = (Index)i;
      b = a.ptr[v];
      e = a.ptr[v + 1];
    }
    const Index len = e > b ? e - b : 0;
    if (len > kLvBlockLen) {
      const unsigned at = atomicAdd(&sl->b, 1u);
      if (at < (unsigned)a.n) publish(&a.longlist[at], v);
    } else if (len > kLvSmallLen) {
      L.big[atomicAdd(&L.nbig, 1)] = v;                                      // (at most one a thread: room for all)
    }
    {                                                                        // ---- a lane a row
      const bool mine = len > 0 && len <= kLvLaneLen;
      if (__ballot(mine) != 0ull) {
        int cu[kLvLaneLen];
        unsigned w[kLvLaneLen], tt[kLvLaneLen];
#pragma unroll
        for (int j = 0; j < kLvLaneLen; ++j) {
          const bool ok = mine && j < len;
          const Index u = ok ? a.ind[b + j] : v;
          const bool in = ok && u != v && (unsigned)u < (unsigned)a.n;
          w[j] = in ? (unsigned)a.val[b + j] : 0u;
          cu[j] = in ? (int)fresh(&a.c[u]) : -1;
        }
        const int ca = mine ? (int)fresh(&a.c[v]) : 0;
        const unsigned kv = mine ? a.k[v] : 0u;
#pragma unroll
        for (int j = 0; j < kLvLaneLen; ++j) tt[j] = cu[j] >= 0 && cu[j] != ca ? fresh(&a.tot[cu[j]]) : 0u;
        unsigned ea = 0;
        long long bs = kLvNone;
        unsigned bx = kLvEmpty;
#pragma unroll
        for (int j = 0; j < kLvLaneLen; ++j) {
          if (cu[j] == ca) ea += w[j];
          if (cu[j] < 0 || cu[j] == ca) continue;
          unsigned ex = 0;
#pragma unroll
          for (int q = 0; q < kLvLaneLen; ++q) ex += cu[q] == cu[j] ? w[q] : 0u;
          lv_better(a.W * (long long)ex - (long long)kv * (long long)tt[j], (unsigned)cu[j], bs, bx);
        }
        if (mine) props += lv_settle(a, v, (Index)ca, kv, ea, bs, bs == kLvNone ? (Index)-1 : (Index)bx);
      }
    }
    unsigned long long mids = __ballot(len > kLvLaneLen && len <= kLvWaveLen);
    while (mids) {                                                           // ---- a wave a row, an entry a lane
      const int l = __ffsll((long long)mids) - 1;
      mids &= mids - 1ull;
      const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
      const Index wb = (Index)__builtin_amdgcn_readlane((int)b, l);
      const int wlen = (int)__builtin_amdgcn_readlane((int)len, l);
      const bool ok = lane < wlen;
      const Index u = ok ? a.ind[wb + lane] : wv;
      const bool in = ok && u != wv && (unsigned)u < (unsigned)a.n;
      const unsigned w = in ? (unsigned)a.val[wb + lane] : 0u;
      const int cu = in ? (int)fresh(&a.c[u]) : -1;
      const int ca = (int)fresh(&a.c[wv]);
      const unsigned kv = a.k[wv];
      const bool cand = cu >= 0 && cu != ca;
      const unsigned tt = cand ? fresh(&a.tot[cu]) : 0u;
      const unsigned ea = wave_sum_u32(cu == ca ? w : 0u);
      unsigned ex = 0;
      for (int q = 0; q < wlen; ++q) {
        const int cq = __shfl(cu, q, kWave);
        const unsigned wq = (unsigned)__shfl((int)w, q, kWave);
        ex += cq == cu ? wq : 0u;
      }
      long long bs = cand ? a.W * (long long)ex - (long long)kv * (long long)tt : kLvNone;
      unsigned bx = cand ? (unsigned)cu : kLvEmpty;
      lv_wave_best(bs, bx);
      if (lane == 0) props += lv_settle(a, wv, (Index)ca, kv, ea, bs, bs == kLvNone ? (Index)-1 : (Index)bx);
    }
    unsigned long long smalls = __ballot(len > kLvWaveLen && len <= kLvSmallLen);
    while (smalls) {                                                         // ---- a wave a row, its slice of the table
      const int l = __ffsll((long long)smalls) - 1;
      smalls &= smalls - 1ull;
      const Index wv = (Index)__builtin_amdgcn_readlane((int)v, l);
      const Index wb = (Index)__builtin_amdgcn_readlane((int)b, l);
      const Index we = (Index)__builtin_amdgcn_readlane((int)e, l);
      const unsigned ca = (unsigned)fresh(&a.c[wv]);
      const unsigned kv = a.k[wv];
      lv_walk<kWave>(a, wv, wb, we, lane, [&](unsigned x, unsigned w) { lv_insert<kLvSmallBits>(wkey, wsum, x, w); });
      __builtin_amdgcn_wave_barrier();
      unsigned ea = 0, bx = kLvEmpty;
      long long bs = kLvNone;
      lv_table_scan<(1 << kLvSmallBits), kWave>(a, wkey, wsum, lane, ca, kv, ea, bs, bx);
      __builtin_amdgcn_wave_barrier();
      lv_wave_best(bs, bx);
      ea = wave_sum_u32(ea);                                                 // (one slot holds the own community)
      if (lane == 0) props += lv_settle(a, wv, (Index)ca, kv, ea, bs, bs == kLvNone ? (Index)-1 : (Index)bx);
    }
    __syncthreads();                                                         // the waves' slices are empty again
    const int nbig = L.nbig;
    for (int r = 0; r < nbig; ++r) {                                         // ---- the workgroup a row, the whole table
      const Index wv = L.big[r];
      const unsigned ca = (unsigned)fresh(&a.c[wv]);
      const unsigned kv = a.k[wv];
      lv_walk<kPThreads>(a, wv, a.ptr[wv], a.ptr[wv + 1], tid, [&](unsigned x, unsigned w) { lv_insert<kLvBlockBits>(s_key, s_sum, x, w); });
      __syncthreads();
      unsigned ea = 0, bx = kLvEmpty;
      long long bs = kLvNone;
      lv_table_scan<kLvSlots, kPThreads>(a, s_key, s_sum, tid, ca, kv, ea, bs, bx);
      lv_block_best(L, tid, lane, wave, bs, bx, ea);
      if (tid == 0) props += lv_settle(a, wv, (Index)ca, kv, ea, bs, bs == kLvNone ? (Index)-1 : (Index)bx);
      __syncthreads();
    }
    __syncthreads();
  }
  return props;
}

// the queued long rows: workgroup b < pool_count takes the rows b, b + pool_count, ... with its own count array
__device__ __forceinline__ unsigned lv_propose_long(const LvArgs& a, unsigned nlong, LvLds& L, int tid, int lane, int wave) {
  unsigned props = 0;
  if ((int)blockIdx.x >= a.pool_count) return 0u;
  unsigned* const E = a.pool + (size_t)blockIdx.x * a.pool_stride;
  for (unsigned i = blockIdx.x; i < nlong; i += (unsigned)a.pool_count) {
    const Index wv = fresh(&a.longlist[i]);
    if ((unsigned)wv >= (unsigned)a.n) continue;                             // (never; the same in every thread)
    const Index wb = a.ptr[wv], we = a.ptr[wv + 1];
    const unsigned ca = (unsigned)fresh(&a.c[wv]);
    const unsigned kv = a.k[wv];
    lv_walk<kPThreads>(a, wv, wb, we, tid, [&](unsigned x, unsigned w) {
      if (w) __hip_atomic_fetch_add(&E[x], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // this wave's adds have landed
    __syncthreads();
    unsigned ea = 0, bx = kLvEmpty;
    long long bs = kLvNone;
    lv_walk<kPThreads>(a, wv, wb, we, tid, [&](unsigned x, unsigned) {
      if (x == ca) return;
      const unsigned ex = fresh(&E[x]), tt = fresh(&a.tot[x]);
      lv_better(a.W * (long long)ex - (long long)kv * (long long)tt, x, bs, bx);
    });
    lv_block_best(L, tid, lane, wave, bs, bx, ea);
    if (tid == 0) props += lv_settle(a, wv, (Index)ca, kv, fresh(&E[ca]), bs, bs == kLvNone ? (Index)-1 : (Index)bx);
    __syncthreads();                                                         // every sum has been read
    lv_walk<kPThreads>(a, wv, wb, we, tid, [&](unsigned x, unsigned) { publish(&E[x], 0u); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                         // the zeros are back before the next row adds
  }
  return props;
}

__global__ __launch_bounds__(kPThreads) void louvain_level_kernel(LvArgs a) {
  __shared__ unsigned s_key[kLvSlots];
  __shared__ unsigned s_sum[kLvSlots];
  __shared__ LvLds s_rows;
  __shared__ unsigned long long s_red[kPWaves][4];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  const long long gwave = (long long)wave * G + blockIdx.x, gwaves = (long long)G * kPWaves;   // neighbouring chunks: different CUs
  LvState* st = a.st;
  const long long n = a.n;
  const bool has_long = st->maxlen[0] > (unsigned)kLvBlockLen && a.pool_count > 0;            // (written before the launch)
  unsigned gen = 0, passes = 0, rounds = 0;
  unsigned long long moves = 0, proposals = 0;
  LvSlot* sl = &st->slot[0];
  for (int s = tid; s < kLvSlots; s += kPThreads) { s_key[s] = kLvEmpty; s_sum[s] = 0u; }
  __syncthreads();

  auto pass_begin = [&]() {
    sl = &st->slot[passes & 3u];
    if (blockIdx.x == 0 && tid == 0) {
      LvSlot* z = &st->slot[(passes + 2u) & 3u];
      publish(&z->a, 0u);
      publish(&z->b, 0u);
      publish(&z->sum, 0ull);
      publish(&z->sum2, 0ull);
    }
  };
  auto pass_end = [&]() -> bool {
    if (!grid_sync(&st->bar, gen, false)) return false;
    ++passes;
    return true;
  };
  // the workgroup's part of a pass's sums, one atomic each
  auto reduce = [&](unsigned x, unsigned long long s1, unsigned long long s2) {
    x = wave_sum_u32(x);
    s1 = wave_sum_u64(s1);
    s2 = wave_sum_u64(s2);
    if (lane == 0) { s_red[wave][0] = x; s_red[wave][1] = s1; s_red[wave][2] = s2; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long bx = 0, b1 = 0, b2 = 0;
      for (int w = 0; w < kPWaves; ++w) { bx += s_red[w][0]; b1 += s_red[w][1]; b2 += s_red[w][2]; }
      if (bx) __hip_atomic_fetch_add(&sl->a, (unsigned)bx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (b1) __hip_atomic_fetch_add(&sl->sum, b1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (b2) __hip_atomic_fetch_add(&sl->sum2, b2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  };

  while (rounds < (unsigned)a.max_rounds) {
    // ---- P: the proposals
    unsigned found = 0;
    {
      pass_begin();
      const unsigned mine = lv_propose(a, sl, s_key, s_sum, s_rows, tid, lane, wave, gwave, gwaves);
      reduce(mine, 0ull, 0ull);
      if (!pass_end()) return;
      found = fresh(&sl->a);
      if (has_long) {
        unsigned nlong = fresh(&sl->b);
        if (nlong > (unsigned)a.n) nlong = (unsigned)a.n;
        pass_begin();
        const unsigned more = lv_propose_long(a, nlong, s_rows, tid, lane, wave);
        reduce(more, 0ull, 0ull);
        if (!pass_end()) return;
        found += fresh(&sl->a);
      }
    }
    ++rounds;
    if (found == 0u) break;                              // a round without proposals: the level's last
    proposals += found;
    // ---- C: who holds a community's largest gain
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const Index d = fresh(&a.prop_d[v]);
      if ((unsigned)d >= (unsigned)a.n) continue;
      const unsigned long long g = fresh(&a.prop_g[v]);
      const Index ca = fresh(&a.c[v]);
      if (fresh(&a.best[ca]) == g) atomicMin(&a.win[ca], (int)v);
      if (fresh(&a.best[d]) == g) atomicMin(&a.win[d], (int)v);
    }
    if (!pass_end()) return;
    // ---- A: accept
    pass_begin();
    for (long long v = gtid; v < n; v += gthreads) {
      const Index d = fresh(&a.prop_d[v]);
      if ((unsigned)d >= (unsigned)a.n) continue;
      const unsigned long long g = fresh(&a.prop_g[v]);
      const Index ca = fresh(&a.c[v]);
      const int wa = fresh(&a.win[ca]), wd = fresh(&a.win[d]);
      bool ok = wa == (int)v;
      if (ok && wd != (int)v) {
        const long long kv = (long long)a.k[v];
        ok = (unsigned)wd < (unsigned)a.n && fresh(&a.prop_d[wd]) == d && (long long)g > kv * ((long long)fresh(&a.K[d]) - kv);
      }
      if (!ok) publish(&a.prop_g[v], 0ull);              // (nobody else reads v's gain in this pass)
    }
    if (!pass_end()) return;
    // ---- U: apply, and what the round touched back to its identities
    {
      unsigned moved = 0;
      pass_begin();
      for (long long v = gtid; v < n; v += gthreads) {
        const Index d = fresh(&a.prop_d[v]);
        if ((unsigned)d >= (unsigned)a.n) continue;
        const Index ca = fresh(&a.c[v]);
        publish(&a.best[ca], 0ull);
        publish(&a.best[d], 0ull);
        publish(&a.win[ca], kLvNoWin);
        publish(&a.win[d], kLvNoWin);
        publish(&a.K[d], 0u);
        if (fresh(&a.prop_g[v]) != 0ull) {
          const unsigned kv = a.k[v];
          publish(&a.c[v], d);
          if (kv) {
            __hip_atomic_fetch_sub(&a.tot[ca], kv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&a.tot[d], kv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          ++moved;
        }
      }
      reduce(moved, 0ull, 0ull);
      if (!pass_end()) return;
      moves += fresh(&sl->a);
    }
  }

  // ---- the record's sums: in(x) over the stored entries (a thread an entry, its row by a search), tot(x)^2 over the communities
  unsigned long long in_sum = 0, tot2 = 0;
  {
    unsigned long long my_in = 0, my_t2 = 0;
    pass_begin();
    for (long long p = gtid; p < a.nnz; p += gthreads) {
      Index lo = 0, hi = a.n;                            // the row: the last r with ptr[r] <= p
      while (hi - lo > 1) {
        const Index mid = lo + ((hi - lo) >> 1);
        if ((long long)a.ptr[mid] <= p) lo = mid; else hi = mid;
      }
      const Index u = a.ind[p];
      if ((unsigned)u < (unsigned)a.n && fresh(&a.c[lo]) == fresh(&a.c[u])) my_in += (unsigned long long)(unsigned)a.val[p];
    }
    for (long long x = gtid; x < n; x += gthreads) {
      const unsigned long long t = fresh(&a.tot[x]);
      my_t2 += t * t;
    }
    reduce(0u, my_in, my_t2);
    if (!pass_end()) return;
    in_sum = fresh(&sl->sum);
    tot2 = fresh(&sl->sum2);
  }
  if (gtid == 0) {
    st->rec[0] = rounds;
    st->rec[1] = moves;
    st->rec[2] = proposals;
    st->rec[3] = passes;
    st->rec[4] = in_sum;
    st->rec[5] = tot2;
    st->rec[kLvDone] = 1ull;
  }
}

// ---- after the levels ----------------------------------------------------------------------------------------------------------
// comp(v) = map(comp(v)): the original vertices follow their vertex of the level into its community's number
__global__ __launch_bounds__(kBlock) void lv_compose_kernel(Index* __restrict__ comp, long long n, const Index* __restrict__ map, Index nl) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) {
    const Index x = comp[v];
    if ((unsigned)x < (unsigned)nl) comp[v] = map[x];
  }
}
__global__ __launch_bounds__(kBlock) void lv_iota_kernel(Index* __restrict__ out, long long n) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock) out[v] = (Index)v;
}
// first(x) = the smallest original vertex of community x (first: INT_MAX before), then labels(v) = first(comp(v))
__global__ __launch_bounds__(kBlock) void lv_first_kernel(const Index* __restrict__ comp, long long n, Index nc, int* __restrict__ first) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock)
    if ((unsigned)comp[v] < (unsigned)nc) atomicMin(&first[comp[v]], (int)v);
}
__global__ __launch_bounds__(kBlock) void lv_labels_kernel(const Index* __restrict__ comp, long long n, Index nc, const int* __restrict__ first,
                                                           int* __restrict__ out) {
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < n; v += (long long)gridDim.x * kBlock)
    out[v] = (unsigned)comp[v] < (unsigned)nc ? first[comp[v]] : (int)v;
}

namespace {

struct MatrixGuard {                // a level's graph, freed on the way out
  grb_matrix m = nullptr;
  ~MatrixGuard() { if (m) (void)grb_matrix_free(m); }
};

grb_info louvain_run(grb_vector labels, grb_matrix A, int weighted, int max_levels, int max_rounds, grb_louvain_result* res) {
  GRB_TRY(ctx_init());
  Context& cx = ctx();
  hipStream_t s = cx.stream;
  const Index n = A->nrows;
  const long long Z = n > 0 ? (long long)A->nvals : 0;
  const int f32 = A->dtype == GRB_F32 ? 1 : 0;
  grb_louvain_result r = {};
  r.levels = 1;
  r.rounds = 1;
  r.communities = n;
  GRB_TRY(dense_out_prepare(labels, n));                 // before anything runs; labels stays as it was until the end
  if (n == 0) {
    GRB_TRY(dense_out_commit(labels, nullptr, 0, s));
    if (res) *res = r;
    return GRB_SUCCESS;
  }
  GRB_TRY(persistent_kernel_fits<louvain_level_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, eleven words per vertex of a level (c, k, tot, prop_d, win, K, the long rows' queue,
  // prop_g and best at two each), the composed assignment and the smallest members, the i32 weights, the partial sums of W
  const size_t st_bytes = pad_bytes(sizeof(LvState));
  const size_t vw = pad_words((size_t)n + 1);
  const size_t zw = pad_words((size_t)Z + 8);
  EwmBuf work, pool;
  GRB_TRY(ewm_alloc(&work, st_bytes + 4 * (13 * vw + zw) + 8 * (size_t)kLvSumBlocks + 256));
  LvArgs a = {};
  a.st = (LvState*)work.p;
  a.prop_g = (unsigned long long*)((char*)work.p + st_bytes);
  a.best = a.prop_g + vw;
  a.c = (Index*)(a.best + vw);
  unsigned* d_k = (unsigned*)(a.c + vw);
  a.k = d_k;
  a.tot = d_k + vw;
  a.prop_d = (Index*)(a.tot + vw);
  a.win = (int*)(a.prop_d + vw);
  a.K = (unsigned*)(a.win + vw);
  a.longlist = (Index*)(a.K + vw);
  Index* d_comp = a.longlist + vw;
  int* d_first = (int*)(d_comp + vw);
  int* d_wbase = d_first + vw;
  unsigned long long* d_partial = (unsigned long long*)(d_wbase + zw);
  double* d_W = (double*)(d_partial + kLvSumBlocks);
  unsigned* d_flag = (unsigned*)(d_W + 1);
  // the weights begin at the same offset inside a 16-byte line as A's indices (an adopted array may begin at any 4-byte
  // boundary): a quad of indices and the quad of their weights are both aligned
  int* d_w = d_wbase + ((reinterpret_cast<uintptr_t>(A->csr.ind) >> 2) & 3u);
  a.pool_count = 0;
  if (n > kLvBlockLen) {                                 // (a row of more than kLvBlockLen entries needs as many columns)
    size_t arrays = kLvPoolBytes / (4 * (size_t)vw);
    if (arrays < 1) arrays = 1;
    if (arrays > (size_t)cx.num_cu) arrays = (size_t)cx.num_cu;
    GRB_TRY(ewm_alloc(&pool, 4 * arrays * vw));
    a.pool = (unsigned*)pool.p;
    a.pool_stride = vw;
    a.pool_count = (int)arrays;
  }
  GRB_TRY(bfs_lanes_fence(s));      // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(d_flag, 0, 8, s));
  if (a.pool_count) GRB_HIP_TRY(hipMemsetAsync(pool.p, 0, 4 * (size_t)a.pool_count * vw, s));
  // ---- the weights, W, the symmetry check: the first read
  long long W = 0;
  if (Z > 0) {
    if (weighted) launch_symmetry_check<true>(A, d_flag + 1, s);
    else launch_symmetry_check<false>(A, d_flag + 1, s);                      // (the values are never read)
    const int blocks = (int)((Z + kBlock - 1) / kBlock < kLvSumBlocks ? (Z + kBlock - 1) / kBlock : kLvSumBlocks);
    hipLaunchKernelGGL(lv_weights_kernel, dim3(blocks), dim3(kBlock), 0, s, (const unsigned*)A->csr.val, Z, weighted, f32, d_w, d_flag, d_partial);
    hipLaunchKernelGGL(weight_final_kernel<false>, dim3(1), dim3(kWave), 0, s, (const unsigned long long*)d_partial, blocks, d_W);
    GRB_HIP_TRY(hipGetLastError());
    struct { double W; unsigned flag[2]; } h;
    GRB_HIP_TRY(hipMemcpyAsync(&h, d_W, sizeof(h), hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
    if (h.flag[1] != 0u) return GRB_INVALID_VALUE;       // A's CSR and CSC differ: not symmetric
    if (h.flag[0] != 0u) return GRB_INVALID_VALUE;       // a weight that is no non-negative integer
    if (h.W > 2147483647.0) return GRB_INVALID_VALUE;    // W > 2^31 - 1
    W = (long long)h.W;
  }
  r.w = W;
  hipLaunchKernelGGL(lv_iota_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_comp, (long long)n);
  GRB_HIP_TRY(hipGetLastError());
  Index nc = n;                                          // the communities so far = the vertices of the current level
  if (W > 0) {
    // ---- the levels.  Level 0 reads A's structure with the i32 weights; a later one the contraction before it
    std::unique_ptr<grb_matrix_s> view(new grb_matrix_s());
    view->dtype = GRB_I32;
    view->nrows = view->ncols = n;
    view->nvals = (Index)Z;
    view->built = true;
    view->owned = false;
    view->format = 1;
    view->csr.ptr = A->csr.ptr;
    view->csr.ind = A->csr.ind;
    view->csr.val = d_w;
    view->csr.n = n;
    view->csr.nvals = (Index)Z;
    grb_matrix cur = view.get();
    MatrixGuard held;
    a.W = W;
    a.max_rounds = max_rounds;
    r.levels = 0;
    r.rounds = 0;
    long long qn = 0;
    for (;;) {
      const Index nl = cur->nrows;
      a.ptr = cur->csr.ptr;
      a.ind = cur->csr.ind;
      a.val = (const int*)cur->csr.val;
      a.n = nl;
      a.nnz = (long long)cur->nvals;
      GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
      hipLaunchKernelGGL(lv_init_kernel, dim3(stream_grid(nl, kWavesPerBlock)), dim3(kBlock), 0, s, a, d_k);
      hipLaunchKernelGGL(louvain_level_kernel, dim3(cx.num_cu), dim3(kPThreads), 0, s, a);
      GRB_HIP_TRY(hipGetLastError());
      unsigned long long h[kLvRec];
      GRB_HIP_TRY(hipMemcpyAsync(h, a.st->rec, sizeof(h), hipMemcpyDeviceToHost, s));
      GRB_HIP_TRY(hipStreamSynchronize(s));              // the level's one read
      if (h[kLvDone] != 1ull) return GRB_PANIC;          // a grid barrier gave up
      ++r.levels;
      ++r.launches;
      r.rounds += (int32_t)h[0];
      r.moves += (int64_t)h[1];
      r.proposals += (int64_t)h[2];
      r.passes += (int32_t)h[3];
      qn = W * (long long)h[4] - (long long)h[5];
      if (h[1] == 0ull) break;                           // a level that moved nothing: the partition is the one before it
      // c becomes map in place, the original vertices follow it
      grb_vector_s cv;
      cv.dtype = GRB_I32;
      cv.nsize = nl;
      cv.vec_type = GRB_DENSE;
      cv.d_val = a.c;
      cv.d_nnz = nl;
      cv.d_owned = false;
      cv.s_owned = false;
      int32_t count = 0;
      GRB_TRY(grb_relabel(&cv, &cv, GRB_RELABEL_LABELS, &count, nullptr));
      hipLaunchKernelGGL(lv_compose_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, d_comp, (long long)n, (const Index*)a.c, nl);
      GRB_HIP_TRY(hipGetLastError());
      nc = (Index)count;
      if (r.levels >= max_levels) break;
      MatrixGuard next;
      GRB_TRY(grb_matrix_new(&next.m, GRB_I32, nc, nc));
      next.m->format = 1;                                // only the CSR is ever read
      GRB_TRY(grb_contract(next.m, nullptr, cur, &cv, GRB_OP_PLUS, 1, nullptr, nullptr));
      if (held.m) (void)grb_matrix_free(held.m);
      held.m = next.m;
      next.m = nullptr;
      cur = held.m;
    }
    r.qn = qn;
    r.modularity = (double)qn / ((double)W * (double)W);
  }
  r.communities = nc;
  // ---- labels(v) = the smallest original vertex of v's community
  GRB_HIP_TRY(hipMemsetAsync(d_first, 0x7f, 4 * (size_t)nc, s));
  hipLaunchKernelGGL(lv_first_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, (const Index*)d_comp, (long long)n, nc, d_first);
  hipLaunchKernelGGL(lv_labels_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, (const Index*)d_comp, (long long)n, nc, (const int*)d_first,
                     (int*)a.tot);                       // (tot is free now)
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  GRB_TRY(dense_out_commit(labels, a.tot, n, s));
  if (res) *res = r;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract is the comment in include/grb_hip.h
grb_info grb_louvain(grb_vector labels, grb_matrix A, int weighted, int max_levels, int max_rounds, grb_descriptor desc,
                     grb_louvain_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!labels || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || labels->nsize != n) return GRB_DIMENSION_MISMATCH;
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || labels->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  if ((weighted != 0 && weighted != 1) || max_levels < 1 || max_rounds < 1) return GRB_INVALID_VALUE;
  if (n > 0 && A->nvals > 0 && !A->csr.ptr) return GRB_INVALID_OBJECT;
  return louvain_run(labels, A, weighted, max_levels, max_rounds, result);
}
