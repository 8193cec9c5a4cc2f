// kcore.hip -- the k-core decomposition on the device: grb_coreness and grb_kcore.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definition is LAGraph's and Gunrock's:
//   core(v) = the largest k such that v is in the k-core, the largest subgraph whose vertices all have k neighbours in it.
//
// The whole peel is ONE co-resident launch (a 1024-thread workgroup per CU, persist_common.hpp's bounded grid barrier
// between its passes); the host reads one record when it is over.
//   deg      i32 per vertex: the neighbours not yet removed.  A vertex is REMOVED exactly when deg <= T, T the threshold
//            of the level being peeled (coreness: T = the level k; kcore: T = k - 1, the one level there is).
//   order    i32 per vertex: every vertex in the order of its removal.  The frontier of a round is order[head, tail);
//            what the round removes is appended behind it, so there is no second queue and nothing to reset, and a
//            vertex is in it once.  A pass reserves room with atomic adds on ITS OWN counter (three in rotation) on top of
//            the tail every workgroup holds: a workgroup that is already in the next pass cannot move the number the
//            slower ones still have to read after the barrier.
//   scan     a pass over deg: lists the vertices with kprev < deg <= want behind the tail and takes the smallest live degree,
//            the live vertices and the sum of their degrees along.  After level k the scan asks for k + 1; when that
//            lists nothing the next level IS the minimum it found and one more scan lists it: an empty level costs
//            nothing, a jump two passes.  The first scan computes deg from the pointers (minus a stored diagonal).
//   round    every frontier vertex's row is walked: a neighbour u with deg[u] > T gets one returning atomic decrement; the
//            thread that sees T + 1 come back has removed u and appends it, a thread that sees <= T adds its one back.
//            deg[u] > T only ever falls and deg[u] <= T is final, so the check before the atomic may be stale (it is
//            read past the L1) and every vertex is appended exactly once; at a barrier every removed vertex of a
//            coreness run holds deg = its level = core(v).
//   rows     of up to kKcLaneLen entries: a lane, four entries in flight; up to kKcWaveLen: a wave, 16-byte index loads;
//            longer: the workgroup.  A round deals the frontier to the WAVES of the grid, one vertex each while there
//            are more waves than vertices, else up to 64.
//   appends  are staged per wave in LDS, kKcStage at a time, and reserved with one atomic per flush.
// The live vertices at the start of level k are the k-core, so the scan that opens the last level has counted the
// kmax-core.  Working memory: deg and order, 8 bytes per vertex, and 2.25 KiB of state, one allocation.
#include "graph_common.hpp"

namespace grb {

constexpr int kKcLaneLen = 8;                            // a row of up to this many entries: one lane walks it
constexpr int kKcWaveLen = 2048;                         // ... up to this many: a wave; longer: the workgroup
constexpr int kKcStage = 256;                            // appends a wave stages in LDS before it reserves room for them
constexpr int kKcRec = 16;

struct KcSlot {                     // what a scan adds up; 128 bytes
  unsigned inv_min;                 // max of ~deg over the live vertices (0: none)
  unsigned live;
  unsigned long long sum;
  unsigned pad[28];
};
struct KcState {                    // zeroed by the host before the launch
  GridBarrier bar;
  unsigned added[3][32];            // what pass p appended: added[p % 3]; workgroup 0 clears added[(p + 1) % 3] meanwhile
  KcSlot slot[4];                   // scan s adds into slot[s & 3]; workgroup 0 clears slot[(s + 2) & 3] meanwhile
  unsigned long long rec[kKcRec];   // [0] edges x 2 [1] result_edges x 2 [2] kmax [3] levels [4] result_vertices [5] passes
                                    // [6] done; [8]: the symmetry check's flag (graph_common.hpp)
};
constexpr int kKcFlag = 8, kKcDone = 6;

struct KcArgs {
  const Index *ptr, *ind;
  Index n;
  int k;                            // < 0: coreness; else the k of kcore
  int* deg;
  Index* order;
  KcState* st;
};

// ---- removing one end of up to N edges: the loads, then the checks, then the atomics, each stage for all N ---------------
template <int N>
__device__ __forceinline__ void kc_hit(const KcArgs& a, const Index (&u)[N], bool (&ok)[N], int T) {
  int d[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok[j] = ok[j] && (unsigned)u[j] < (unsigned)a.n;
    d[j] = ok[j] ? fresh(&a.deg[u[j]]) : T;
  }
  int old[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ok[j] = ok[j] && d[j] > T;
    old[j] = ok[j] ? atomicSub(&a.deg[u[j]], 1) : T;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (ok[j] && old[j] <= T) atomicAdd(&a.deg[u[j]], 1);                   // removed meanwhile: not this thread's to take
    ok[j] = ok[j] && old[j] == T + 1;                                        // this thread removed u[j]
  }
}

// the row [b, e) walked by kThreads threads (t: this one's number among them); every lane of every wave of them calls it
template <int kThreads>
__device__ __forceinline__ void kc_walk(const KcArgs& a, Index b, Index e, int t, int lane, int T, WaveStage& o) {
  const QuadSpan s = quad_span(a.ind, b, e);
  const Index b4 = s.b4, nq = s.nq, te = s.te, nh = s.nh, ns = s.ns;
  if (kThreads == kWave || t < kWave) {
    Index u[1] = {0};
    bool ok[1] = {t < ns};
    if (ok[0]) u[0] = a.ind[t < nh ? b + t : te + (t - nh)];
    kc_hit<1>(a, u, ok, T);
    stage_push<kKcStage>(o, lane, ok[0], u[0]);
  }
  for (Index q0 = 0; q0 < nq; q0 += kThreads) {
    const Index q = q0 + t;
    bool ok[4];
    ok[0] = ok[1] = ok[2] = ok[3] = q < nq;
    const int4 c = ok[0] ? *reinterpret_cast<const int4*>(a.ind + b4 + 4 * (long long)q) : make_int4(0, 0, 0, 0);
    const Index u[4] = {c.x, c.y, c.z, c.w};
    kc_hit<4>(a, u, ok, T);
#pragma unroll
    for (int j = 0; j < 4; ++j) stage_push<kKcStage>(o, lane, ok[j], u[j]);
  }
}

__global__ __launch_bounds__(kPThreads) void kcore_persistent_kernel(KcArgs a) {
  __shared__ Index s_stage[kPWaves][kKcStage];
  __shared__ Index s_big[kPThreads];
  __shared__ int s_nbig;
  __shared__ unsigned long long s_red[kPWaves][3];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int G = gridDim.x;
  const long long gtid = (long long)blockIdx.x * kPThreads + tid;
  const long long gthreads = (long long)G * kPThreads;
  const long long gwave = (long long)wave * G + blockIdx.x, gwaves = (long long)G * kPWaves;   // neighbouring chunks: different CUs
  KcState* st = a.st;
  if (*reinterpret_cast<const unsigned int*>(&st->rec[kKcFlag]) != 0u) return;   // not symmetric: every workgroup reads the same word
  WaveStage o = {s_stage[wave], 0u, a.order, &st->added[0][0], 0u, (unsigned)a.n};   // base: the queue's length when the pass began
  unsigned gen = 0;
  const bool peel_all = a.k < 0;
  const long long n = a.n;

  // kprev < deg: live.  A scan lists kprev < deg <= want
  int kprev = -1, want = peel_all ? 0 : a.k - 1;
  unsigned head = 0, tail = 0;
  unsigned scans = 0, passes = 0, levels = 0;
  // a pass begins: its counter, the next one's cleared; and ends: the barrier, then what it appended
  auto pass_begin = [&]() {
    o.counter = &st->added[passes % 3u][0];
    o.base = tail;
    if (blockIdx.x == 0 && tid == 0) publish(&st->added[(passes + 1u) % 3u][0], 0u);
  };
  auto pass_end = [&]() -> bool {
    stage_flush(o, lane);
    if (!grid_sync(&st->bar, gen, false)) return false;
    tail += fresh(o.counter);
    if (tail > (unsigned)a.n) tail = (unsigned)a.n;
    ++passes;
    return true;
  };
  unsigned long long edges2 = 0, level_sum = 0;
  unsigned level_live = 0;
  int kmax = 0;

  // one scan; -> the smallest live degree (~0u: nothing is live), the live vertices, the sum of their degrees
  // final_pass: kcore's last pass instead: deg < k becomes 0, the others are counted
  auto scan = [&](bool first, bool final_pass, unsigned& mn, unsigned& live, unsigned long long& sum) -> bool {
    KcSlot* sl = &st->slot[scans & 3u];
    pass_begin();
    if (blockIdx.x == 0 && tid == 0) {
      KcSlot* z = &st->slot[(scans + 2u) & 3u];
      publish(&z->inv_min, 0u);
      publish(&z->live, 0u);
      publish(&z->sum, 0ull);
    }
    unsigned my_inv = 0, my_live = 0;
    unsigned long long my_sum = 0;
    for (long long base = 0; base < n; base += gthreads) {
      const long long v = base + gtid;
      const bool ok = v < n;
      int d = 0;
      if (ok) {
        if (first) { d = row_degree_no_diag(a.ptr, a.ind, (Index)v); publish(&a.deg[v], d); }
        else d = fresh(&a.deg[v]);
      }
      bool alive = ok && d > kprev;
      if (final_pass) {
        alive = ok && d >= a.k;
        if (ok && !alive) a.deg[v] = 0;
      }
      if (alive) {
        const unsigned inv = ~(unsigned)d;
        my_inv = inv > my_inv ? inv : my_inv;
        ++my_live;
        my_sum += (unsigned long long)d;
      }
      if (!final_pass) stage_push<kKcStage>(o, lane, alive && d <= want, (Index)v);
    }
    stage_flush(o, lane);
    my_inv = wave_max_u32(my_inv);
    my_live = wave_sum_u32(my_live);
    my_sum = wave_sum_u64(my_sum);
    if (lane == 0) { s_red[wave][0] = my_inv; s_red[wave][1] = my_live; s_red[wave][2] = my_sum; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long bi = 0, bl = 0, bs = 0;
      for (int w = 0; w < kPWaves; ++w) { bi = s_red[w][0] > bi ? s_red[w][0] : bi; bl += s_red[w][1]; bs += s_red[w][2]; }
      if (bl) {
        __hip_atomic_fetch_max(&sl->inv_min, (unsigned)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&sl->live, (unsigned)bl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&sl->sum, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (!pass_end()) return false;
    mn = ~fresh(&sl->inv_min);
    live = fresh(&sl->live);
    sum = fresh(&sl->sum);
    ++scans;
    return true;
  };

  for (;;) {
    unsigned mn, live;
    unsigned long long sum;
    if (!scan(scans == 0, false, mn, live, sum)) return;
    if (scans == 1) edges2 = sum;                        // (kprev = -1: every vertex is live)
    if (live == 0u) break;
    if (tail == head) {                                  // nothing at `want`
      if (!peel_all) break;
      want = (int)mn;                                    // the next level there is
      continue;
    }
    // ---- level `want` begins; what is live is its core
    const int T = want;
    ++levels;
    kmax = want;
    level_sum = sum;
    level_live = live;
    while (tail > head) {
      const unsigned F = tail - head, end = tail;
      pass_begin();
      const unsigned per = F >= (unsigned long long)gwaves * kWave ? (unsigned)kWave : (unsigned)((F + gwaves - 1) / gwaves);
      for (long long c0 = 0; c0 * per < F; c0 += gwaves) {
        if (tid == 0) s_nbig = 0;
        __syncthreads();
        const long long i = (c0 + gwave) * per + lane;
        const bool have = lane < (int)per && i < (long long)F;
        Index v = 0, b = 0, e = 0;
        if (have) {
          v = fresh(&a.order[head + (unsigned)i]);
          if ((unsigned)v < (unsigned)a.n) { b = a.ptr[v]; e = a.ptr[v + 1]; }
        }
        const Index len = e - b;
        if (len > kKcWaveLen) s_big[atomicAdd(&s_nbig, 1)] = v;              // (at most one a thread: room for all)
        {                                                                    // the short rows, a lane each
          const bool mine = len <= kKcLaneLen;
          const unsigned longest = wave_max_u32(mine && len > 0 ? (unsigned)len : 0u);
          for (Index j0 = 0; j0 < (Index)longest; j0 += 4) {
            Index u[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ok[j] = mine && j0 + j < len;
              u[j] = ok[j] ? a.ind[b + j0 + j] : 0;
            }
            kc_hit<4>(a, u, ok, T);
#pragma unroll
            for (int j = 0; j < 4; ++j) stage_push<kKcStage>(o, lane, ok[j], u[j]);
          }
        }
        unsigned long long mids = __ballot(len > kKcLaneLen && len <= kKcWaveLen);
        while (mids) {                                                       // the wave's rows, one after the other
          const int l = __ffsll((long long)mids) - 1;
          mids &= mids - 1ull;
          kc_walk<kWave>(a, (Index)__builtin_amdgcn_readlane((int)b, l), (Index)__builtin_amdgcn_readlane((int)e, l), lane, lane, T, o);
        }
        __syncthreads();
        const int nbig = s_nbig;
        for (int r = 0; r < nbig; ++r) {                                     // the workgroup's rows
          const Index w = s_big[r];
          kc_walk<kPThreads>(a, a.ptr[w], a.ptr[w + 1], tid, lane, T, o);
        }
        __syncthreads();
      }
      if (!pass_end()) return;
      head = end;
    }
    kprev = want;
    if (!peel_all || head >= (unsigned)a.n) break;       // kcore has one level; nobody is left
    want = kprev + 1;
  }

  unsigned long long res_edges2 = level_sum;
  unsigned res_vertices = level_live;
  if (!peel_all) {                                       // what survived: deg >= k
    unsigned mn, live;
    unsigned long long sum;
    if (!scan(false, true, mn, live, sum)) return;
    res_edges2 = sum;
    res_vertices = live;
    kmax = a.k;
    levels = 1;
  }
  if (gtid == 0) {
    st->rec[0] = edges2;
    st->rec[1] = res_edges2;
    st->rec[2] = (unsigned long long)(unsigned)kmax;
    st->rec[3] = levels;
    st->rec[4] = res_vertices;
    st->rec[5] = passes;
    st->rec[kKcDone] = 1ull;
  }
}

namespace {

grb_info kcore_empty(grb_vector out, int k, grb_kcore_result* res) {       // n = 0
  GRB_TRY(ctx_init());
  GRB_TRY(grb_vector_set_storage(out, GRB_DENSE));
  out->d_nnz = 0;
  grb_kcore_result none = {};
  if (k >= 0) { none.kmax = k; none.levels = 1; }
  if (res) *res = none;
  return GRB_SUCCESS;
}

grb_info kcore_run(grb_vector out, grb_matrix A, int k, grb_kcore_result* res) {
  GRB_TRY(ctx_init());
  Context& c = ctx();
  hipStream_t s = c.stream;
  const Index n = A->nrows;
  GRB_TRY(persistent_kernel_fits<kcore_persistent_kernel>());
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- one allocation: the state, deg, order
  const size_t st_bytes = pad_bytes(sizeof(KcState));
  const size_t vw = pad_words((size_t)n);
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, st_bytes + 8 * vw));
  KcArgs a;
  a.ptr = A->csr.ptr;
  a.ind = A->csr.ind;
  a.n = n;
  a.k = k;
  a.st = (KcState*)work.p;
  a.deg = (int*)((char*)work.p + st_bytes);
  a.order = (Index*)(a.deg + vw);
  GRB_TRY(dense_out_prepare(out, n));                    // before anything runs; out stays as it was until the end

  GRB_TRY(bfs_lanes_fence(s));      // a whole-device grid must not meet a BFS lane's narrower one half-way (bfs_persist.hip)
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  GRB_HIP_TRY(hipMemsetAsync(work.p, 0, st_bytes, s));
  launch_symmetry_check<false>(A, (unsigned int*)&a.st->rec[kKcFlag], s);
  hipLaunchKernelGGL(kcore_persistent_kernel, dim3(c.num_cu), dim3(kPThreads), 0, s, a);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  unsigned long long h_rec[kKcRec];
  GRB_HIP_TRY(hipMemcpyAsync(h_rec, a.st->rec, sizeof(h_rec), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // the call's one read
  if ((unsigned int)h_rec[kKcFlag] != 0u) return GRB_INVALID_VALUE;         // A's CSR and CSC differ: not symmetric
  if (h_rec[kKcDone] != 1ull) return GRB_PANIC;                              // a grid barrier gave up
  GRB_TRY(dense_out_commit(out, a.deg, n, s));
  grb_kcore_result r = {};
  r.edges = (int64_t)(h_rec[0] / 2);
  r.result_edges = (int64_t)(h_rec[1] / 2);
  r.kmax = (int32_t)h_rec[2];
  r.levels = (int32_t)h_rec[3];
  r.result_vertices = (int32_t)h_rec[4];
  r.rounds = (int32_t)h_rec[5];
  r.launches = 1;
  GRB_HIP_TRY(hipEventElapsedTime(&r.loop_ms, ev.a, ev.b));
  if (res) *res = r;
  return GRB_SUCCESS;
}

// k < 0: coreness
grb_info kcore_entry(grb_vector out, grb_matrix A, bool all_levels, int k, grb_kcore_result* result) {
  if (!out || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  const Index n = A->nrows;
  if (A->nrows != A->ncols || out->nsize != n) return GRB_DIMENSION_MISMATCH;
  if (all_levels) k = -1;
  else if (k < 0) return GRB_INVALID_VALUE;
  if (out->dtype != GRB_I32 || (A->dtype != GRB_F32 && A->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (n == 0) return kcore_empty(out, k, result);
  if (!A->csr.ptr) return GRB_INVALID_OBJECT;
  return kcore_run(out, A, k, result);
}

}  // namespace
}  // namespace grb

using namespace grb;

// the contract of both is the comment in include/grb_hip.h
grb_info grb_coreness(grb_vector core, grb_matrix A, grb_descriptor desc, grb_kcore_result* result) { GRB_API_ENTER();
  (void)desc;
  return kcore_entry(core, A, true, 0, result);
}

grb_info grb_kcore(grb_vector v, grb_matrix A, int k, grb_descriptor desc, grb_kcore_result* result) { GRB_API_ENTER();
  (void)desc;
  return kcore_entry(v, A, false, k, result);
}
