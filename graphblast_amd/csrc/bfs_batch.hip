// bfs_batch.hip -- up to 64 traversals at once: the multi-frontier form of algorithm::bfs.
//
// In GraphBLAS terms a level of k simultaneous traversals is  F' = (A^T lor.land F) .* not(Seen)
// with F, Seen : n x k Boolean -- the sparse x dense product the reference leaves as a stub
// (backend/cuda/operations.hpp:52-70, spmm.hpp:15-27).  With k <= 64 a row of F is ONE 64-bit
// word (bit s = "in the frontier of source s"), the semiring's add is a word-wide OR, its
// multiply the AND with the edge's presence: one 8-byte gather per edge serves 64 traversals.
// No tile of A is dense enough for a matrix core to beat that (the dense-core SpMM path that
// tried was measured slower and removed in round 5).
//
//   seen[v], W_L[v]  one 64-bit word per vertex; W_L = the bits discovered by level L, kept for
//                    the first kStore levels (the frontier of level L + 1 IS W_L)
//   direction        chosen PER SOURCE every level from that source's frontier size and out-degree
//                    sum: bits of small frontiers are pushed, bits of large ones pulled, in the same
//                    level.  (A union rule makes every vertex scan its whole list for the 63 sources
//                    that are still near their start while one hub source already floods the graph.)
//   pull (bits Q)    a lane per vertex: need = ~seen & Q; the hinted in-neighbour first, four serial
//                    probes, then the wave finishes its open rows together in rounds (each row's next 32,
//                    128, 512 ... entries laid end to end and dealt evenly to the lanes, ORed per row in
//                    LDS), a row stopping once every needed bit is found.  Rows of >= 4096 entries are
//                    cut into 4096-entry slices taken by separate waves
//   push (bits P)    frontier words with P bits expand along out-edges, the edges of a wave's 64 vertices dealt
//                    evenly to its lanes: an atomicOr into seen claims the unseen bits, a second into W_L
//                    records them (the pull pass has just written every word of W_L; zeroed when nothing is
//                    pulled); a streaming pass then counts the pushed bits of W_L per source
//   labels           not written while traversing: one final pass turns the stored level words into
//                    the k depth vectors (label[s][v] = level of discovery, source = 1, unreached =
//                    0) with full-width coalesced stores -- no memset, no scattered 4-byte stores.
//                    Levels beyond kStore (long-diameter graphs, tiny frontiers) label directly.
//                    The vectors are what k calls of algorithm::bfs return: BFS depth is unique.
#include "bfs_kernels.hpp"
#include "persist_common.hpp"
#include "batch_decide.hpp"
#include "batch_slots.hpp"
#include <chrono>
#include <climits>

namespace grb {

constexpr int kBatchBig = 4096;       // row length from which a row is cut into slices (GRB_BATCH_BIG_IN / _OUT)
constexpr int kBatchBigPush = 512;    // the same for out-edge rows: a pushed edge costs more than a pulled one
constexpr int kBatchSlice = 4096;     // pull: entries per slice, at most
constexpr int kBatchPushSlice = 1024; // push: out-edge slices (every edge is a chain of dependent memory steps)
constexpr int kBatchSerial = 4;       // serial probes per lane before the wave takes over
constexpr int kBatchSlots = 16;       // counter slots (spreads same-address atomics)
constexpr int kBatchStoreMax = 16;    // level words kept for the final label pass
constexpr int kBatchCounters = 2 + 128 + 2;   // per slot: vertices, the big in-rows still open (below), {nf_s, mf_s} per source, big out-rows found, U (below)
constexpr int kCntInOpen = 1, kCntBigOut = 2 + 128, kCntOpenU = 2 + 128 + 1;
static_assert(kBatchCounters <= kBlock, "batch_totals_kernel sums a counter per thread");
static_assert(kBatchStoreMax + 1 == kSlotsKeptMax, "batch_slots.hpp records a level per kept slot");
constexpr int kBatchBoxPer = kBatchCounters + 9;      // the host's box: where the light-level launch leaves TailState::cum and ::last
constexpr int kBoxDecision = kBatchCounters + 5;      // box: {qmask, pmask, kind, stash} of the NEXT level, as batch_totals_kernel decided it
constexpr int kBatchCtlWords = 5;                     // the device's copy of the first three, behind the counter slots; [3]: the last light-level launch's status; [4]: stash
constexpr int kCtlStash = 4;
// The big-row list of an owner-computes level is kept in kListSegs parts, each with a length on a line of its own: a wave
// of batch_push_kernel appends to part (workgroup index mod kListSegs).  With ONE length the ~1500 waves that list a row
// at RMAT-22 queued behind one address (5 ns an update: 7 us on the push kernel, measured); the owners read the parts
// end to end.
constexpr int kListSegs = 8;
constexpr int kListLenStride = 32;                    // unsigned ints between two lengths: 128 bytes
constexpr size_t kListHeader = (size_t)kListSegs * kListLenStride * sizeof(unsigned int);
// counter kCntInOpen: the big in-rows that still lack a bit of some source (fewer than 2^31: a row index is an int), with
// bit 62 set when the level's batch_big_apply_kernel counted them at all; counter kCntBigOut: the vertices with a new bit
// whose out-row is big
constexpr unsigned long long kInOpenCounted = 1ull << 62;
// counter kCntOpenU: U, the in-edges of the rows a level's pull leaves open -- a row that still lacks a bit of some source
// in qmask adds its whole in-degree (batch_pull_kernel for the rows it finishes itself, batch_big_apply_kernel for the
// rows of the slice kernels).  It bounds what the next level's pull can inspect for those sources.  It is COMPLETE only
// when the level pulled every live source (pmask = 0, qmask != 0): batch_totals_kernel then publishes it with bit 62 set,
// and only then may the finishing rule (batch_decide.hpp) read it.  At most nvals, far below 2^62.
constexpr unsigned long long kOpenUComplete = 1ull << 62;
constexpr int kBatchBoxWords = kBatchBoxPer + 128 + 64;

typedef unsigned long long u64;

struct BatchArgs {
  const Index *optr, *oind, *iptr, *iind;
  const Index* hint;
  Index n;
  u64 qmask, pmask;                   // bits pulled / pushed this level
  u64* seen;
  const u64* fcur;
  u64* fnext;
  int big;                            // rows of this many entries or more belong to the slice kernels
  int big_out;                        // ... the same for out-rows, whichever direction the kernel works in: what batch_commit_l counts
  int claims;                         // heavy push levels: the push kernels claim in seen and nothing else; the commit pass finds the new bits
  u64 stash;                          // the bit columns of fnext that carry the pushed sources' OLD seen-bits from the pull pass to the commit
                                      // pass: pmask on a heavy level, else 0 (batch_decide_stash)
  const int* big_index;               // batch_push_kernel on an owner-computes level: vertex -> big index, for the list (else null)
  int* list;                          // ... the list it appends the skipped big frontier rows to: {big index, pushed frontier bits}, part g at g * nbig
  u64* list_fw;
  const int4* slices;                 // {vertex, first entry, end entry, big index}
  int nslices;
  const Index* bigrows;               // the big rows' vertex ids
  int nbig;
  u64* counters;                      // [kBatchSlots][kBatchCounters]
  float new_label;
  int direct_labels;                  // levels beyond the stored ones write labels as they discover
  int k;
  unsigned int* list_len;             // the big-row list's kListSegs lengths (kListLenStride apart): appended to by batch_push_kernel, put back to
                                      // zero for the next level by batch_push_commit_kernel behind the owner kernels (else null)
  const u64* ctl;                     // a launch made ahead of the host: {qmask, pmask, kind, -, stash} as the level before decided them (else null)
  float* label[64];
};

struct LabelArgs {
  Index n;
  int k, nstored;
  const u64* seen;
  const u64* go;                      // launched ahead of the host, behind a light-level launch: that launch's status (else null)
  const u64* W[kBatchStoreMax + 1];   // the stored levels' words ...
  float lab[kBatchStoreMax + 1];      // ... and the depth each of them assigns (0: the level the iteration cap cuts off)
  float* label[64];
};

__device__ inline u64 wave_or(u64 x) { return wave_or_u64(x); }   // DPP (common.hpp): twelve LDS-crossbar permutes otherwise

// the bits a pull kernel works on; false: launched ahead of a level that turned out to be none of the host loop's --
// nothing is read or written (grid-uniform: every workgroup leaves before its first barrier)
__device__ inline bool batch_pull_bits(const BatchArgs& a, u64& q, u64& stash) {
  q = a.qmask;
  stash = a.stash;
  if (!a.ctl) return true;
  if (a.ctl[2] != (u64)kDecideHost) return false;
  q = a.ctl[0];
  stash = a.ctl[kCtlStash];
  return true;
}
__device__ inline bool batch_pull_bits(const BatchArgs& a, u64& q) {
  u64 stash;
  return batch_pull_bits(a, q, stash);
}

struct BatchTotals {                  // per workgroup, in LDS
  u64 v[kBatchCounters];
};

#ifndef GRB_BATCH_TRANSPOSE_FROM
#define GRB_BATCH_TRANSPOSE_FROM 8
#endif
constexpr int kTransposeFrom = GRB_BATCH_TRANSPOSE_FROM;     // live sources in a wave from which the bit matrix is transposed by exchanges

// A wave's running totals, source s in lane s: nf = (vertex, source) pairs discovered, mf = their out-degrees
struct WaveTotals {
  u64 nf = 0, mf = 0;
  unsigned int verts = 0;             // wave-uniform: vertices with any new bit
  unsigned int bigs = 0;              // wave-uniform: those of them whose out-row is big (the next level's push has slices to expand)
  u64 open_in = 0;                    // per lane: the in-degrees of the rows this lane's pull left open (counter kCntOpenU); only the pull kernels add to it
};

// accounting (and, beyond the stored levels, labels) of a lane's new bits; wave-collective.  The 64 x 64 bit
// matrix (lane = vertex, bit = source) is transposed with one ballot per live source, so lane s holds the
// mask m of vertices new to source s: nf_s += popcount(m), and the degree sum comes from the degrees' bit
// planes, mf_s += sum_b 2^b popcount(m & plane_b) -- all 64 sources in parallel, no per-source reduction.
// (count_big = false: the light-level kernel, at 121 of the 128 VGPRs its 1024-thread workgroups may use, does not pay
// for a count nobody reads -- after its hand-back the host launches the push helpers unconditionally)
__device__ inline void batch_commit_l(const BatchArgs& a, WaveTotals& acc, Index v, u64 newb, bool direct, float label,
                                      bool count_big = true) {
  const unsigned long long mv = __ballot(newb != 0);
  if (!mv) return;
  const int lane = lane_id();
  acc.verts += (unsigned int)__popcll(mv);
  unsigned int deg = 0;
  if (newb) deg = (unsigned int)(a.optr[v + 1] - a.optr[v]);
  if (count_big) acc.bigs += (unsigned int)__popcll(__ballot(deg >= (unsigned int)a.big_out));
  u64 m = 0;
  const u64 live = wave_or(newb);
  if (__popcll(live) <= kTransposeFrom) {
    for (u64 t = live; t; t &= t - 1) {
      const int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)t) - 1);   // wave-uniform: a scalar index
      const unsigned long long col = __ballot((newb >> s) & 1ull);
      if (lane == s) m = col;
    }
  } else {
    // many live sources: the 64 x 64 bit matrix is transposed in six exchange steps (blocks of 32, 16, ... 1 swapped
    // with the lane `k` away) instead of one ballot per source -- ~70 instructions against ~10 per source
    m = newb;
    auto exchange = [&](int k, u64 keep) {
      const u64 y = __shfl_xor(m, k, kWave);
      m = (lane & k) ? ((m & ~keep) | ((y >> k) & keep)) : ((m & keep) | ((y << k) & ~keep));
    };
    exchange(32, 0x00000000ffffffffull);
    exchange(16, 0x0000ffff0000ffffull);
    exchange(8, 0x00ff00ff00ff00ffull);
    exchange(4, 0x0f0f0f0f0f0f0f0full);
    exchange(2, 0x3333333333333333ull);
    exchange(1, 0x5555555555555555ull);
  }
  acc.nf += (u64)__popcll(m);
  unsigned int dor = deg;
  dor = wave_or_u32(dor);
  for (unsigned int t = dor; t; t &= t - 1) {
    const int b = __builtin_amdgcn_readfirstlane(__ffs((int)t) - 1);
    const unsigned long long plane = __ballot((deg >> b) & 1u);
    acc.mf += (u64)__popcll(m & plane) << b;
  }
  if (direct)
    for (u64 t = newb; t; t &= t - 1) a.label[__ffsll((long long)t) - 1][v] = label;
}
__device__ inline void batch_commit(const BatchArgs& a, WaveTotals& acc, Index v, u64 newb) {
  batch_commit_l(a, acc, v, newb, a.direct_labels != 0, a.new_label);
}

__device__ inline void totals_init(BatchTotals* lds) {
  for (int i = threadIdx.x; i < kBatchCounters; i += blockDim.x) lds->v[i] = 0;
  __syncthreads();
}
// (with_open: the two pull kernels that count U; a literal at every call, so nobody else pays for the wave sum)
__device__ inline void totals_flush_to(u64* slots, BatchTotals* lds, const WaveTotals& acc, bool with_open = false) {
  const int lane = lane_id();
  if (acc.nf) atomicAdd(&lds->v[2 + 2 * lane], acc.nf);
  if (acc.mf) atomicAdd(&lds->v[3 + 2 * lane], acc.mf);
  if (lane == 0 && acc.verts) atomicAdd(&lds->v[0], (u64)acc.verts);
  if (lane == 0 && acc.bigs) atomicAdd(&lds->v[kCntBigOut], (u64)acc.bigs);
  if (with_open) {
    const u64 open_in = wave_sum_u64(acc.open_in);          // one LDS update per wave, one per workgroup and slot below: no atomic per row
    if (lane == 0 && open_in) atomicAdd(&lds->v[kCntOpenU], open_in);
  }
  __syncthreads();
  u64* dst = slots + (size_t)(blockIdx.x & (kBatchSlots - 1)) * kBatchCounters;
  for (int i = threadIdx.x; i < kBatchCounters; i += blockDim.x)
    if (lds->v[i]) atomicAdd(&dst[i], lds->v[i]);
}
__device__ inline void totals_flush(const BatchArgs& a, BatchTotals* lds, const WaveTotals& acc, bool with_open = false) {
  totals_flush_to(a.counters, lds, acc, with_open);
}

// the wave scans entries [rs, re) of `ind`, ORs word[ind[q]] and stops once `nd` is covered
__device__ inline u64 wave_scan_or(const Index* __restrict__ ind, const u64* __restrict__ word, Index rs, Index re,
                                   u64 nd, int lane) {
  u64 got = 0;
  for (Index q = rs; q < re; q += 4 * kWave) {
    u64 w = 0;
    Index c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Index at = q + j * kWave + lane;
      c[j] = at < re ? ind[at] : -1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= c[j] >= 0 ? word[c[j]] : 0ull;
    got |= wave_or(w);
    if ((got & nd) == nd) break;
  }
  return got;
}

// the sources come as kernel arguments (no host-to-device copy in front of a sweep).  w0 != nullptr: the seeds are a
// stored level of their own; else a source's own label is written here and no word array holds the seeds (the label
// pass leaves a pair that is seen but in no stored level alone)
struct SeedSources { Index v[64]; };
struct SeedLabels { float* p[64]; };
__global__ __launch_bounds__(kBlock) void batch_seed_kernel(u64* seen, u64* w0, SeedSources src, SeedLabels label, int k) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < k) {
    const Index v = src.v[s];
    atomicOr(&seen[v], 1ull << s);
    if (w0) atomicOr(&w0[v], 1ull << s);
    else label.p[s][v] = 1.0f;
  }
}

// ---- the sweep's first level when every source is pushed ----------------------------------------------------------
// The frontier is the k sources, whose rows the host knows: no queue, no scan, no co-resident grid.  A row is cut into
// pieces of kFirstPiece edges, source s owning pieces pre[s] .. pre[s + 1] (the prefix sums come by value), a wave per
// piece: consecutive pieces on consecutive workgroups, so a hub's row spreads over every XCD.  A discovery is one
// returning atomicOr on seen; the claimed bit goes into the level's words (all-zero before the launch) and is counted
// as in every host-level kernel.  A vertex named twice is two sources with the same row.
constexpr int kFirstPiece = 4 * kWave;
struct FirstPieces { unsigned int pre[65]; };
static_assert(kFirstPiece == 256, "a wave takes a piece's edges four per lane");
__global__ __launch_bounds__(kBlock) void batch_first_level_kernel(BatchArgs a, SeedSources src, FirstPieces fp) {
  __shared__ BatchTotals lds;
  totals_init(&lds);
  WaveTotals tot;
  const int lane = lane_id();
  const unsigned int piece = blockIdx.x * kWavesPerBlock + wave_id();
  if (piece < fp.pre[a.k]) {                                // wave-uniform
    int s = 0;                                              // the last source whose first piece is <= piece
#pragma unroll
    for (int step = 32; step > 0; step >>= 1)
      if (s + step < a.k && fp.pre[s + step] <= piece) s += step;
    const Index u = src.v[s];
    const u64 bit = 1ull << s;
    const Index p = a.optr[u] + (Index)(piece - fp.pre[s]) * kFirstPiece, re = a.optr[u + 1];
    const Index e = re - p > kFirstPiece ? p + kFirstPiece : re;
    Index dst[4];
    u64 nb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Index at = p + j * kWave + lane;
      dst[j] = at < e ? a.oind[at] : -1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) nb[j] = dst[j] >= 0 ? (bit & ~atomicOr(&a.seen[dst[j]], bit)) : 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (nb[j]) atomicOr(&a.fnext[dst[j]], nb[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) batch_commit_l(a, tot, nb[j] ? dst[j] : 0, nb[j], a.direct_labels != 0, a.new_label);
  }
  totals_flush(a, &lds, tot);
}

__global__ __launch_bounds__(kBlock) void batch_pull_kernel(BatchArgs a) {
  __shared__ BatchTotals lds;
  __shared__ Index s_pre[kWavesPerBlock][kWave];
  __shared__ Index s_p[kWavesPerBlock][kWave];
  __shared__ u64 s_acc[kWavesPerBlock][kWave];
  // Heavy level (stash = pmask != 0): every store of the level's word also carries the vertex's OLD seen-bits of the
  // pushed sources, in their own bit columns -- disjoint from qmask, so batch_pull_slices_kernel and
  // batch_big_apply_kernel, which mask what they read of fnext with qmask, never see them; the push kernels of such a
  // level do not touch fnext, and batch_push_commit_kernel takes the columns back (new = seen & pmask & ~stashed).
  u64 qmask, stash;
  if (!batch_pull_bits(a, qmask, stash)) return;
  if (qmask == 0) {                                         // every live source is pushed: the push kernels OR into all-zero words
    for (Index v = (Index)blockIdx.x * blockDim.x + threadIdx.x; v < a.n; v += (Index)gridDim.x * blockDim.x)
      a.fnext[v] = stash ? (a.seen[v] & stash) : 0ull;      // (grid-uniform: seen is read on a heavy level only)
    return;
  }
  totals_init(&lds);
  WaveTotals tot;
  const int lane = lane_id(), w = wave_id();
  const Index nchunks = (a.n + kWave - 1) / kWave;
  const Index nwaves = (Index)gridDim.x * kWavesPerBlock;
  for (Index chunk = (Index)blockIdx.x * kWavesPerBlock + wave_id(); chunk < nchunks; chunk += nwaves) {
    const Index v = chunk * kWave + lane;
    const bool valid = v < a.n;
    const u64 seen = valid ? a.seen[v] : ~0ull;
    u64 need = ~seen & qmask;
    Index p = 0, e = 0;
    if (need) { p = a.iptr[v]; e = a.iptr[v + 1]; }
    const Index indeg = e - p;
    const bool big = indeg >= a.big;                       // probed here, finished by the slice kernels
    if (p == e) need = 0;
    if (__ballot(need != 0) == 0ull) {
      if (valid) a.fnext[v] = seen & stash;
      continue;
    }
    u64 acc = 0;
    if (need && a.hint) acc = a.fcur[a.hint[v]];
#pragma unroll
    for (int t = 0; t < kBatchSerial; ++t) {
      const bool go = need && (acc & need) != need && p < e;
      const Index c = a.iind[go ? p : 0];
      const u64 w = a.fcur[go ? c : 0];
      if (go) { acc |= w; ++p; }
    }
    // the rows still open finish together: round by round each takes its next `quota` entries (32, 128, 512, ...),
    // the entries of all of them are laid end to end and dealt to the lanes 256 at a time, the gathered
    // words are ORed per row in LDS -- full lanes whatever the row lengths, an exit test per row per round
    Index quota = 32;
    for (;;) {
      const bool open = !big && need && (acc & need) != need && p < e;
      if (__ballot(open) == 0ull) break;
      const Index cnt = open ? (e - p < quota ? e - p : quota) : 0;
      Index inc = cnt;
inc = (Index)wave_incl_scan_u32((unsigned)inc);
      const Index total = __shfl(inc, kWave - 1, kWave);
      __builtin_amdgcn_wave_barrier();
      s_pre[w][lane] = inc - cnt;
      s_p[w][lane] = p;
      s_acc[w][lane] = 0ull;
      __builtin_amdgcn_wave_barrier();
      for (Index base = 0; base < total; base += 4 * kWave) {
        Index c[4];
        int row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const Index at = base + j * kWave + lane;
          c[j] = -1; row[j] = 0;
          if (at < total) {
            int r = 0;                                     // the last row whose first entry is <= at
#pragma unroll
            for (int step = kWave / 2; step > 0; step >>= 1)
              if (s_pre[w][r + step] <= at) r += step;
            row[j] = r;
            c[j] = a.iind[s_p[w][r] + (at - s_pre[w][r])];
          }
        }
        u64 wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = c[j] >= 0 ? a.fcur[c[j]] : 0ull;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (wv[j]) atomicOr(&s_acc[w][row[j]], wv[j]);
      }
      __builtin_amdgcn_wave_barrier();
      acc |= s_acc[w][lane];
      p += cnt;
      if (quota < (1 << 20)) quota *= 4;
    }
    const u64 newb = acc & need;
    if (valid) {
      a.fnext[v] = newb | (seen & stash);                  // a big row's probe result: the slices add to it,
      if (newb && !big) a.seen[v] = seen | newb;           // batch_big_apply_kernel claims and counts it
    }
    if (!big && (need & ~newb)) tot.open_in += (u64)indeg;  // left open: the row's in-edges are part of U (a big row's: batch_big_apply_kernel)
    batch_commit(a, tot, valid ? v : 0, big ? 0ull : newb);
  }
  totals_flush(a, &lds, tot, true);
}

// pull, big rows: a wave per 4096-entry slice
__global__ __launch_bounds__(kBlock) void batch_pull_slices_kernel(BatchArgs a) {
  const int lane = lane_id();
  const int nwaves = gridDim.x * kWavesPerBlock;
  u64 qmask;
  if (!batch_pull_bits(a, qmask) || qmask == 0) return;
  for (int sl = blockIdx.x * kWavesPerBlock + wave_id(); sl < a.nslices; sl += nwaves) {
    const int4 S = a.slices[sl];
    const u64 need = ~a.seen[S.x] & qmask & ~a.fnext[S.x];   // what the probes (and other slices) left open
    if (!need) continue;
    const u64 got = wave_scan_or(a.iind, a.fcur, S.y, S.z, need, lane) & need;
    if (lane == 0 && got) atomicOr(&a.fnext[S.x], got);
  }
}

__global__ __launch_bounds__(kBlock) void batch_big_apply_kernel(BatchArgs a) {
  __shared__ BatchTotals lds;
  u64 qmask;
  if (!batch_pull_bits(a, qmask) || qmask == 0) return;
  totals_init(&lds);
  WaveTotals tot;
  const int nthreads = gridDim.x * blockDim.x;
  // the big in-rows that still lack a bit of any of the k sources: it never rises, and once it is 0 no pull level has
  // anything left for the slice kernels or for this one (the host stops launching them)
  const u64 all = a.k >= 64 ? ~0ull : (1ull << a.k) - 1ull;
  unsigned int open = 0;
  for (int base = 0; base < a.nbig; base += nthreads) {
    const int b = base + blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = b < a.nbig;
    const Index v = valid ? a.bigrows[b] : 0;
    u64 newb = 0, left = 0;
    if (valid) {
      const u64 seen = a.seen[v];
      newb = a.fnext[v] & ~seen & qmask;
      if (newb) a.seen[v] = seen | newb;
      left = ~(seen | newb) & all;
      if (left & qmask) tot.open_in += (u64)(a.iptr[v + 1] - a.iptr[v]);   // this level's pull leaves it open: its share of U
    }
    open += (unsigned int)__popcll(__ballot(left != 0ull));
    batch_commit(a, tot, v, newb);
  }
  if (lane_id() == 0) {
    const u64 add = (u64)open + (blockIdx.x == 0 && threadIdx.x == 0 ? kInOpenCounted : 0ull);
    if (add) atomicAdd(&lds.v[kCntInOpen], add);
  }
  totals_flush(a, &lds, tot, true);
}

// N out-edge slots of frontier vertices (entry q[j] < 0 = empty) carrying the pushed bits fw[j]: the dependent
// steps are issued stage by stage (targets, seen words, the claim in seen, a fire-and-forget OR of the claimed
// bits into fnext) -- one chain of memory latencies per N edges.  The claimed pairs are counted (and, beyond
// the stored levels, labelled) by batch_push_commit_kernel, which reads them back from fnext in one streaming
// pass instead of two random row-pointer reads and LDS atomics per pair here.
template <int N>
__device__ inline void batch_push_slots(const BatchArgs& a, const Index* __restrict__ ind, const Index (&q)[N],
                                        const u64 (&fw)[N]) {
  Index dst[N];
  u64 bits[N];
#pragma unroll
  for (int j = 0; j < N; ++j) dst[j] = q[j] >= 0 ? ind[q[j]] : -1;
#pragma unroll
  for (int j = 0; j < N; ++j) bits[j] = dst[j] >= 0 ? (fw[j] & ~a.seen[dst[j]]) : 0ull;
  if (a.claims) {
    // heavy level: the claim alone, fire and forget -- one random line per edge; the commit pass finds the
    // claimed bits as seen & pmask & ~(the old bits stashed in fnext)
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (bits[j]) atomicOr(&a.seen[dst[j]], bits[j]);
    return;
  }
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (bits[j]) bits[j] &= ~atomicOr(&a.seen[dst[j]], bits[j]);
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (bits[j]) atomicOr(&a.fnext[dst[j]], bits[j]);
}

// push, rows below kBatchBig: the out-edges of a wave's 64 vertices are laid end to end (prefix sum of the
// degrees in LDS) and dealt to the lanes 256 at a time, so a wave pays one chain of memory latencies per 256
// edges whatever the row lengths are
__global__ __launch_bounds__(kBlock) void batch_push_kernel(BatchArgs a) {
  __shared__ Index s_pre[kWavesPerBlock][kWave];
  __shared__ Index s_p[kWavesPerBlock][kWave];
  __shared__ u64 s_fw[kWavesPerBlock][kWave];
  const int lane = lane_id(), w = wave_id();
  const Index nchunks = (a.n + kWave - 1) / kWave;
  const Index nwaves = (Index)gridDim.x * kWavesPerBlock;
  for (Index chunk = (Index)blockIdx.x * kWavesPerBlock + w; chunk < nchunks; chunk += nwaves) {
    const Index u = chunk * kWave + lane;
    const u64 fw = u < a.n ? (a.fcur[u] & a.pmask) : 0ull;
    if (__ballot(fw != 0) == 0ull) continue;
    Index p = 0, e = 0;
    if (fw) { p = a.optr[u]; e = a.optr[u + 1]; }
    const bool skipped = e - p >= a.big;                   // the slice kernel, or the owners, expand it
    if (skipped) p = e;
    if (a.big_index) {                                     // owner-computes level: the owners' list, one length update per wave
      const unsigned long long m = __ballot(skipped);
      if (m) {
        const unsigned int seg = blockIdx.x & (kListSegs - 1);
        unsigned int b0 = 0;
        if (lane == 0) b0 = atomicAdd(&a.list_len[seg * kListLenStride], (unsigned int)__popcll(m));
        b0 = __shfl(b0, 0, kWave);
        if (skipped) {                                     // (a part holds at most every big row once: nbig entries)
          const size_t at = (size_t)seg * (size_t)a.nbig + b0 + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
          a.list[at] = a.big_index[u];
          a.list_fw[at] = fw;                              // the owners read (row, bits) in one step, not three
        }
      }
    }
    const Index d = e - p;
    Index inc = d;
inc = (Index)wave_incl_scan_u32((unsigned)inc);
    const Index total = __shfl(inc, kWave - 1, kWave);
    __builtin_amdgcn_wave_barrier();
    s_pre[w][lane] = inc - d;
    s_p[w][lane] = p;
    s_fw[w][lane] = fw;
    __builtin_amdgcn_wave_barrier();
    for (Index base = 0; base < total; base += 4 * kWave) {
      Index q[4];
      u64 f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const Index at = base + j * kWave + lane;
        q[j] = -1; f[j] = 0ull;
        if (at < total) {
          int r = 0;                                       // the last row whose first edge is <= at
#pragma unroll
          for (int step = kWave / 2; step > 0; step >>= 1)
            if (s_pre[w][r + step] <= at) r += step;
          q[j] = s_p[w][r] + (at - s_pre[w][r]);
          f[j] = s_fw[w][r];
        }
      }
      batch_push_slots<4>(a, a.oind, q, f);
    }
  }
}

__global__ __launch_bounds__(kBlock) void batch_push_slices_kernel(BatchArgs a) {
  const int lane = lane_id();
  const int nwaves = gridDim.x * kWavesPerBlock;
  for (int sl = blockIdx.x * kWavesPerBlock + wave_id(); sl < a.nslices; sl += nwaves) {
    const int4 S = a.slices[sl];
    const u64 fw = a.fcur[S.x] & a.pmask;
    if (!fw) continue;
    for (Index base = S.y + lane; base < S.z; base += 4 * kWave) {
      Index q[4];
      u64 f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const Index at = base + j * kWave;
        q[j] = at < S.z ? at : -1;
        f[j] = fw;
      }
      batch_push_slots<4>(a, a.oind, q, f);
    }
  }
}

// ---- heavy push levels, the big rows by destination range ----------------------------------------------------------
// A heavy level pushes tens of millions of edges, nearly all of them out of a few thousand hub rows, and every edge
// was one atomicOr on a random 8-byte word of the 33 MB `seen` array: ~45 G edges/s, 290 us for the 15 M edges of
// RMAT-22's second level.  The rows are sorted, so a row's entries that fall into one range of destinations are one
// contiguous piece: a workgroup OWNS a range, keeps its words in LDS (at most 8 Ki of them, 64 KiB), ORs into them
// the pieces of every big frontier row (offsets per (row, range) precomputed once per matrix), and writes the range
// back with plain coalesced stores.  No global atomics, every edge read once: 293 -> 105 us for that level's big rows.
constexpr int kOwnRows = 8192;         // 64 KiB of LDS: two workgroups of 1024 per CU
constexpr int kOwnSmallRows = 2048;

// The offsets table is row-major, off[bi * S + b] = where big row bi enters range b, with the stride S = R + 1 rounded
// up to 32 entries: a row's offsets start on a 128-byte line, and the two an owner needs for a list entry (b and b + 1)
// are neighbours.  A heavy level has a few per cent of the big rows in its frontier, in arbitrary order (the vertex ids
// are permuted, the list is appended to with atomics), so the range-major table this replaces gave an owner two lines
// per list entry with one useful word each -- most of the wide instance's HBM traffic; here a list entry's line is
// shared by the owners of the 32 neighbouring ranges, which run at the same time.
static inline long long own_off_stride(long long R) { return (R + 1 + 31) & ~31ll; }

__global__ void batch_range_off_kernel(const Index* __restrict__ optr, const Index* __restrict__ oind,
                                       const Index* __restrict__ bigrows, int nbig, int R, int S, const Index* __restrict__ bounds,
                                       Index* __restrict__ off) {
  const long long total = (long long)nbig * (R + 1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int bi = (int)(i / (R + 1)), b = (int)(i % (R + 1));
    const Index u = bigrows[bi];
    Index lo = optr[u], hi = optr[u + 1];
    const long long key = (long long)bounds[b];            // first entry with a destination >= key
    while (lo < hi) {
      const Index mid = lo + (hi - lo) / 2;
      if ((long long)oind[mid] < key) lo = mid + 1; else hi = mid;
    }
    off[(size_t)bi * S + b] = lo;                          // b fastest: neighbouring threads store neighbouring words (the padding is never read)
  }
}

// The list of a level's big frontier rows, {big index, pushed frontier bits}, is written by batch_push_kernel, which
// reads every frontier word and every frontier row's extent anyway and skips exactly these rows (BatchArgs::big_index:
// the per-matrix table vertex -> big index), in kListSegs parts; batch_push_commit_kernel, behind the owners, puts their
// lengths back to zero.
// A power-law graph sends a fifth of all edges to its first 16 Ki vertices: the ranges are cut at equal in-degree
// mass (at most 8 Ki rows each), so the hub region is many narrow ranges.  (Equal-width ranges with the heavy ones
// shared between several workgroups -- each with its own LDS copy, written back with atomicOr -- were measured
// first: 115-130 us.)  A lane takes a list entry: the piece of one big row inside the range; the pieces of a wave's
// entries are laid end to end and dealt to the lanes.  Two instantiations: the narrow ranges of the hub region
// (<= 2 Ki rows, 16 KiB of LDS, 512 threads: four workgroups per CU -- a workgroup's work is a short chain of
// dependent steps, and with one per CU the chip mostly waits) and the wide ones (two per CU): 27 + 77 us.
template <int kRows, int kThreads>
__global__ __launch_bounds__(kThreads) void batch_push_owner_kernel(BatchArgs a, const Index* __restrict__ range_off, int S,
                                                                    const int* __restrict__ list, const u64* __restrict__ list_fw,
                                                                    const unsigned int* __restrict__ count, const Index* __restrict__ bounds,
                                                                    const int* __restrict__ ids) {
  __shared__ u64 acc[kRows];
  __shared__ Index s_pre[kThreads / kWave][kWave];
  __shared__ Index s_p[kThreads / kWave][kWave];
  __shared__ u64 s_fw[kThreads / kWave][kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int b = ids[blockIdx.x];
  const Index base = bounds[b];
  const int rows = (int)(bounds[b + 1] - base);
  for (int i = tid; i < rows; i += kThreads) acc[i] = 0ull;
  __syncthreads();
  // where each part of the list starts when they are laid end to end: wave-uniform, kept in scalar registers (the wide
  // instance's LDS is exactly half a CU's: a word more and one workgroup fits where two did)
  unsigned int seg0[kListSegs + 1];
  seg0[0] = 0u;
#pragma unroll
  for (int g = 0; g < kListSegs; ++g) seg0[g + 1] = seg0[g] + count[g * kListLenStride];
  const long long nlist = (long long)seg0[kListSegs];
  for (long long k0 = 0; k0 < nlist; k0 += kThreads) {
    const long long i = k0 + tid;
    Index o0 = 0, o1 = 0;
    u64 fw = 0ull;
    if (i < nlist) {
      int g = 0;                                            // the last part that starts at or before i (never an empty one)
      unsigned int g0 = 0u;
#pragma unroll
      for (int t = 1; t < kListSegs; ++t)
        if (seg0[t] <= (unsigned int)i) { g = t; g0 = seg0[t]; }
      const size_t at = (size_t)g * (size_t)a.nbig + (size_t)((unsigned int)i - g0);
      const int bi = list[at];
      fw = list_fw[at];
      o0 = range_off[(size_t)bi * S + b];                   // neighbours: one line per list entry
      o1 = range_off[(size_t)bi * S + b + 1];
    }
    // the pieces of a wave's 64 entries laid end to end and dealt to the lanes 256 edges at a time (as batch_push_kernel
    // does with rows): a wave pays one chain of memory latencies per 256 edges whatever the piece lengths are
    const Index len = o1 - o0;
    Index inc = len;
inc = (Index)wave_incl_scan_u32((unsigned)inc);
    const Index total = __shfl(inc, kWave - 1, kWave);
    if (total == 0) continue;
    const int w = tid >> 6;
    __builtin_amdgcn_wave_barrier();
    s_pre[w][lane] = inc - len;
    s_p[w][lane] = o0;
    s_fw[w][lane] = fw;
    __builtin_amdgcn_wave_barrier();
    constexpr int kPer = 8;                                // edges per lane and step: that many loads in flight
    for (Index at0 = 0; at0 < total; at0 += kPer * kWave) {
      Index q[kPer], d[kPer];
      u64 f[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const Index at = at0 + j * kWave + lane;
        q[j] = -1; f[j] = 0ull;
        if (at < total) {
          int r = 0;                                       // the last entry whose first edge is <= at
#pragma unroll
          for (int step = kWave / 2; step > 0; step >>= 1)
            if (s_pre[w][r + step] <= at) r += step;
          q[j] = s_p[w][r] + (at - s_pre[w][r]);
          f[j] = s_fw[w][r];
        }
      }
#pragma unroll
      for (int j = 0; j < kPer; ++j) d[j] = q[j] >= 0 ? a.oind[q[j]] - base : -1;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (d[j] >= 0) atomicOr(&acc[d[j]], f[j]);
    }
  }
  __syncthreads();
  for (int i = tid; i < rows; i += kThreads) {
    const Index v = base + i;
    const u64 x = acc[i];
    if (x != 0ull) {
      const u64 sv = a.seen[v];
      if (x & ~sv) a.seen[v] = sv | x;                     // the claim; the commit pass finds it against the stashed old bits
    }
  }
}

// after the push kernels of a level: the pushed bits that arrived in fnext are this level's discoveries.  Heavy level
// (claims only): fnext's P columns hold the pushed sources' seen-bits as the pull pass found them, so what the push
// kernels claimed is seen & P & ~old; the columns are rewritten with exactly that -- every stashed bit is cleared, and
// the level's words are the discoveries again before the next level or the label pass reads them.
__global__ __launch_bounds__(kBlock) void batch_push_commit_kernel(BatchArgs a) {
  __shared__ BatchTotals lds;
  totals_init(&lds);
  if (a.list_len && blockIdx.x == 0 && threadIdx.x < kListSegs) a.list_len[threadIdx.x * kListLenStride] = 0u;   // the owner kernels in front of this launch have read them
  WaveTotals tot;
  const int lane = lane_id();
  const Index nchunks = (a.n + kWave - 1) / kWave;
  const Index nwaves = (Index)gridDim.x * kWavesPerBlock;
  for (Index chunk = (Index)blockIdx.x * kWavesPerBlock + wave_id(); chunk < nchunks; chunk += nwaves) {
    const Index v = chunk * kWave + lane;
    u64 pb = 0;
    if (v < a.n) {
      if (a.claims) {
        const u64 w = a.fnext[v], old = w & a.pmask;
        pb = a.seen[v] & a.pmask & ~old;
        if (old | pb) a.fnext[v] = (w & ~a.pmask) | pb;
      } else {
        pb = a.fnext[v] & a.pmask;
      }
    }
    if (__ballot(pb != 0) == 0ull) continue;
    batch_commit(a, tot, pb ? v : 0, pb);
  }
  totals_flush(a, &lds, tot);
}

// the depth vectors from the stored level words: full 256-byte stores, every element written once
__global__ __launch_bounds__(kBlock) void batch_labels_kernel(LabelArgs a) {
  __shared__ float s_lab[32];
  if (a.go && *a.go == 2ull) return;                        // the launch handed a level back: the sweep goes on, nothing is read or written (grid-uniform)
  if (threadIdx.x < 32) s_lab[threadIdx.x] = threadIdx.x >= 1 && (int)threadIdx.x <= a.nstored ? a.lab[threadIdx.x - 1] : 0.f;
  __syncthreads();
  const int lane = lane_id();
  const Index nchunks = (a.n + kWave - 1) / kWave;
  const Index nwaves = (Index)gridDim.x * kWavesPerBlock;
  for (Index chunk = (Index)blockIdx.x * kWavesPerBlock + wave_id(); chunk < nchunks; chunk += nwaves) {
    const Index v = chunk * kWave + lane;
    const bool valid = v < a.n;
    // which stored level found the vertex (1-based, <= kBatchStoreMax + 1 < 32) as five bit planes: plane b holds,
    // per source, bit b of that number (the level words are disjoint, so OR composes them); 0 = none of them
    u64 plane[5] = {0, 0, 0, 0, 0}, hit = 0;
    for (int L = 0; L < a.nstored; ++L) {
      const u64 w = valid ? a.W[L][v] : 0ull;
      hit |= w;
#pragma unroll
      for (int b = 0; b < 5; ++b) plane[b] |= (((L + 1) >> b) & 1) ? w : 0ull;
    }
    const u64 later = valid ? (a.seen[v] & ~hit) : ~0ull;  // seen, but by a level that labelled as it went
    for (int s = 0; s < a.k; ++s) {
      int idx = 0;
#pragma unroll
      for (int b = 0; b < 5; ++b) idx |= (int)((plane[b] >> s) & 1ull) << b;
      if (!((later >> s) & 1ull)) a.label[s][v] = s_lab[idx];
    }
  }
}

// the level's totals summed over the counter slots (left zero for the next level) and published to the host:
// box[0 .. kBatchCounters) the totals, box[kBatchCounters] the level's sequence number, written last
//
// ... and the NEXT level decided here, from the totals just summed, by the rule the host uses (batch_decide.hpp): a lane
// per source.  The decision goes to the control block behind the counters, where pull kernels launched ahead of the
// host find it, and into the box, where the host reads it: one authority, nobody computes it a second time.  The
// finishing rule is applied here and nowhere else in a running sweep: lane 0 has both masks and the level's U, which
// the host marks complete when the level pulled every live source.
struct DecideArgs {
  BatchRule rule;
  int iteration_left;                 // the level decided on may run at all
  int open_complete;                  // the level just run pulled every live source (pmask = 0, qmask != 0): its U is complete.  The host
                                      // knows the level's masks whoever decided them -- it read them from the box
  u64* ctl;
};
// ---- the hot block ---------------------------------------------------------------------------------------------------
// A pulled entry is a random line of the frontier words, and most entries name few vertices: on RMAT-22 the 64 Ki
// vertices of largest out-degree are 62 % of the CSC entries, each alone on its 128-byte line among fifteen cold words.
// Their words are kept a second time, side by side behind the n words of every array a pull can read as its frontier
// (0.5 MiB for 64 Ki hubs: an eighth of an XCD's L2), and the pull kernels gather through copies of the CSC indices and
// of the hint that name hub j as n + j.  The vertex numbering, the probe order and every result stay what they are.  The
// tail must be current before a pull reads the array: the copy below runs between the array's last writer and that
// pull, in stream order.  Measured (docs/experiments.md R26): level 3's pull fetches half the bytes and runs 151 -> 124 us
// at K = 32; the levels bound by dependent latency do not move.
struct HotCopy {
  u64* words;                         // the level's words, n of them, and H more behind them
  const Index* hubs;
  Index n, H;                         // H = 0: nothing to copy
};
__device__ inline void batch_hot_copy(const HotCopy& h, Index first, Index stride) {
  for (Index j = first; j < h.H; j += stride) h.words[(size_t)h.n + j] = h.words[h.hubs[j]];
}
// ... as a launch of its own, where no totals launch sits between the writer and the pull (the seed kernel before a first
// level that pulls, a light-level launch that hands a level back)
__global__ __launch_bounds__(kBlock) void batch_hot_refresh_kernel(HotCopy h) {
  batch_hot_copy(h, (Index)blockIdx.x * blockDim.x + threadIdx.x, (Index)gridDim.x * blockDim.x);
}
constexpr int kHotCopyBlocks = 512;   // at most; 256 words each per round
static inline int hot_copy_blocks(Index H) { return H > 0 ? std::min<int>(ceil_div(H, kBlock), kHotCopyBlocks) : 0; }

// Workgroup 0 sums and decides; the others (hot_copy_blocks of them) bring the tail of the level's words up to date -- they
// cannot know what is decided, so they always copy.
__global__ __launch_bounds__(kBlock) void batch_totals_kernel(u64* counters, u64* box, u64 seq, DecideArgs d, HotCopy hot) {
  __shared__ u64 s_nf[64], s_mf[64], s_open;
  if (blockIdx.x > 0) {
    batch_hot_copy(hot, (Index)(blockIdx.x - 1) * blockDim.x + threadIdx.x, (Index)(gridDim.x - 1) * blockDim.x);
    return;
  }
  const int i = threadIdx.x;
  if (i < kBatchCounters) {
    u64 t = 0;
    for (int slot = 0; slot < kBatchSlots; ++slot) {
      t += counters[slot * kBatchCounters + i];
      counters[slot * kBatchCounters + i] = 0ull;
    }
    if (i == kCntOpenU) {
      s_open = t;
      if (d.open_complete) t |= kOpenUComplete;
    }
    __hip_atomic_store(&box[i], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (i >= 2 && i < 2 + 128) ((i & 1) ? s_mf : s_nf)[(i - 2) >> 1] = t;
  }
  __syncthreads();
  if (i < kWave) {
    const u64 under = __ballot(batch_decide_under(s_nf, i, d.rule));
    const int way = batch_decide_source(s_nf, s_mf, i, d.rule, under);
    u64 q = __ballot(way == 2), p = __ballot(way == 1);
    u64 pushed = wave_sum_u64(way == 1 ? s_mf[i] : 0ull);   // integers below 2^53: the host's sum of doubles is the same number
    if (i == 0) {
      // the finishing rule: few in-edges left open by a level that pulled everybody -- the sources the base rule would
      // push are pulled with the rest, and the level has no push stage
      if (batch_decide_finish(q, p, d.rule, d.open_complete ? (long long)s_open : kOpenUnknown)) { q |= p; p = 0; pushed = 0; }
      const u64 kind = (u64)batch_decide_kind(q, p, (double)pushed, d.rule, d.iteration_left != 0);
      const u64 stash = batch_decide_stash(p, (double)pushed, d.rule.n, (int)kind);
      d.ctl[0] = q; d.ctl[1] = p; d.ctl[2] = kind; d.ctl[kCtlStash] = stash;
      __hip_atomic_store(&box[kBoxDecision], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&box[kBoxDecision + 1], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&box[kBoxDecision + 2], kind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&box[kBoxDecision + 3], stash, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __threadfence_system();
  __syncthreads();
  if (i == 0) __hip_atomic_store(&box[kBatchCounters], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the light levels in one launch ----------------------------------------------------------------------------------
// A level that pushes a few thousand edges costs what its launches cost: four kernels over all n words, a totals
// kernel and a host round trip -- 45-100 us for microseconds of work, on every level of a sweep's tail (and on EVERY
// level of a high-diameter graph, where 64 small frontiers never grow; a sweep's first level, whose frontier the host
// knows, is batch_first_level_kernel's, and a launch that follows it starts from that level's kept words).  While every live
// source is pushed and the level's out-edges stay under a limit, the levels run inside one co-resident launch
// instead: the frontier is a QUEUE of {vertex, first edge} pieces (rows cut at kTailPiece edges, so a hub that turns
// up is shared by many waves), a wave lays the edges of 64 pieces end to end and deals them to its lanes, a claimed
// target gets its bits ORed into the next level's words, and whoever finds that word zero appends the target to the
// next queue.  The words a level read are cleaned through its queue while the following level runs (three word arrays
// in rotation: a word holds bits of several sources, and a vertex one source reached two levels ago may be claimed by
// another right now -- the cleaner and the claimers must not share an array): no memset, no pass over n words after
// the first.
// Labels are written as the pairs are claimed (few of them, by definition); totals per source go through the same
// wave transposition as everywhere else.  One grid barrier per level.
constexpr int kTailPiece = 256;        // edges per queue entry: one step of a wave
constexpr int kTailList = 4096;        // a workgroup's list of newly claimed vertices (beyond it a wave queues its own)
constexpr int kTailLong = 64;          // ... of rows of more than eight pieces

constexpr int kTailStates = 4;         // state blocks zeroed by one fill at a sweep's start: a launch takes the next clean one
struct TailState {                    // all-zero when a launch starts
  GridBarrier bar;
  unsigned int count[4][32];          // queue lengths (one line each; [2..3]: the out-edges queued): level j reads [j & 3], appends to [(j + 1) & 3]
  u64 slots[3][kBatchSlots * kBatchCounters];
  u64 ts[64];                         // GRB_BATCH_TRACE: wall-clock stamps of workgroup 0 (100 MHz)
  u64 dec[3][8][16];                  // what the level loop decides on: {pairs, out-edges} of a level, one line per eighth of the grid
  u64 cum[128];                       // TailArgs::per_source: {pairs, out-edges} per source summed over the launch's levels ...
  unsigned int last[64];              // ... and the last iteration at which the source discovered anything (0: never)
};

struct TailArgs {
  const u64* f0;                      // frontier words of the level before (a stored level: read, never cleaned)
  u64* X[3];                          // all-zero on entry: level j writes X[j % 3], reads X[(j - 1) % 3] and cleans X[(j - 2) % 3]
  u64* queue[3];                      // entries (first edge << 32 | vertex), vertex complemented on all but a row's first piece
  TailState* st;
  u64* box;                           // host-coherent: the last level's totals, then {seq, levels, edges, pairs, status}
  u64* status;                        // the device's copy of the status, for a label pass enqueued behind this launch
  u64 seq;
  int iter0, max_niter;
  unsigned long long edge_limit;      // leave when the next level would push more out-edges than this
  int per_source;                     // the caller wants every source's own totals (the queue's sweep): box[kBatchBoxPer ..]
};

__global__ __launch_bounds__(kPThreads) void batch_tail_kernel(BatchArgs a, TailArgs t) {
  __shared__ BatchTotals lds;
  __shared__ Index s_pre[kPWaves][kWave];
  __shared__ Index s_p[kPWaves][kWave];
  __shared__ u64 s_fw[kPWaves][kWave];
  __shared__ u64 s_sum[kBatchCounters];
  __shared__ u64 s_dec[2];
  __shared__ Index s_list[kTailList];                       // vertices this workgroup was the first to claim this level
  __shared__ unsigned int s_nlist, s_wp[kPWaves], s_we[kPWaves], s_base, s_nlong;
  __shared__ unsigned long long s_before;
  __shared__ int4 s_long[kTailLong];                        // {vertex, first edge, pieces, where}: rows the whole workgroup writes
  const int lane = lane_id(), w = threadIdx.x / kWave;
  const unsigned int gw = blockIdx.x * kPWaves + w, nw = gridDim.x * kPWaves;
  const unsigned int gt = blockIdx.x * kPThreads + threadIdx.x, nt = gridDim.x * kPThreads;
  TailState* st = t.st;
  unsigned gen = 0;
  int nts = 0;
  auto stamp = [&] { if (blockIdx.x == 0 && threadIdx.x == 0 && nts < 64) st->ts[nts++] = wall_clock64(); };
  stamp();

  // wave-collective: every lane brings up to N vertices (v[i] < 0: none); one counter update per call for the whole
  // wave (a level that discovers 300 K vertices would otherwise queue behind 300 K updates of one address).  The
  // out-edges queued so far are counted as well: once they pass the limit the launch is going to hand the next level
  // back to the host, which reads the words, not the queue -- nothing more is written (the level that ends a sweep's
  // first launch discovers rows with 16 M out-edges: 60 K pieces nobody would read).  Rows of more than four pieces are
  // written by the whole wave.
  auto enqueue = [&](u64* q, unsigned int* cnt, const Index (&v)[4], int N) {
    Index p[4];
    unsigned int pieces[4], mine = 0, mine_edges = 0;
    for (int i = 0; i < N; ++i) {
      pieces[i] = 0; p[i] = 0;
      if (v[i] >= 0) {
        p[i] = a.optr[v[i]];
        const Index e = a.optr[v[i] + 1];
        pieces[i] = e > p[i] ? (unsigned int)((e - p[i] + kTailPiece - 1) / kTailPiece) : 1u;   // an empty row is queued too: its word must be cleaned
        mine += pieces[i];
        mine_edges += (unsigned int)(e - p[i]);
      }
    }
    if (__ballot(mine != 0u) == 0ull) return;
    unsigned int inc = mine, ince = mine_edges;
inc = (unsigned int)wave_incl_scan_u32((unsigned)inc);
ince = (unsigned int)wave_incl_scan_u32((unsigned)ince);
    unsigned int base = 0;
    unsigned long long before = 0;
    if (lane == kWave - 1) {
      base = atomicAdd(cnt, inc);
      before = atomicAdd((unsigned long long*)(cnt + 2), (unsigned long long)ince);
    }
    base = __shfl(base, kWave - 1, kWave);
    before = __shfl(before, kWave - 1, kWave);
    if (before > t.edge_limit) return;
    unsigned int at = base + inc - mine;
    for (int i = 0; i < N; ++i) {
      if (pieces[i] <= 4u)
        for (unsigned int c = 0; c < pieces[i]; ++c)
          publish(&q[at + c], ((u64)(unsigned int)(p[i] + (Index)c * kTailPiece) << 32) | (u64)(unsigned int)(c == 0 ? v[i] : ~v[i]));
      for (unsigned long long mk = __ballot(pieces[i] > 4u); mk; mk &= mk - 1) {
        const int l = __ffsll((long long)mk) - 1;
        const Index vv = __shfl(v[i], l, kWave), pp = __shfl(p[i], l, kWave);
        const unsigned int np = __shfl(pieces[i], l, kWave), aa = __shfl(at, l, kWave);
        for (unsigned int c = lane; c < np; c += kWave)
          publish(&q[aa + c], ((u64)(unsigned int)(pp + (Index)c * kTailPiece) << 32) | (u64)(unsigned int)(c == 0 ? vv : ~vv));
      }
      at += pieces[i];
    }
  };

  // The queue's length is one word: a wave per piece (what keeps a level's latency short) would mean a same-address
  // update per piece -- 5 ns each, 50 us for a level of 5 K pieces, measured.  So the waves of a workgroup collect
  // what they claim in LDS and the workgroup takes its room in the queue with ONE update per level; only a wave that
  // finds the LDS list full queues by itself.
  auto collect = [&](u64* q, unsigned int* cnt, const Index (&v)[4], int N) {
    unsigned int mine = 0;
    for (int i = 0; i < N; ++i) mine += v[i] >= 0 ? 1u : 0u;
    if (__ballot(mine != 0u) == 0ull) return;
    unsigned int inc = mine;
inc = (unsigned int)wave_incl_scan_u32((unsigned)inc);
    unsigned int base = 0;
    if (lane == kWave - 1) base = atomicAdd(&s_nlist, inc);
    base = __shfl(base, kWave - 1, kWave);
    const unsigned int total = __shfl(inc, kWave - 1, kWave);
    unsigned int at = base + inc - mine;
    Index rest[4] = {-1, -1, -1, -1};
    for (int i = 0; i < N; ++i)
      if (v[i] >= 0) {
        if (at < (unsigned int)kTailList) s_list[at] = v[i]; else rest[i] = v[i];   // the list stays dense up to its capacity
        ++at;
      }
    if (base + total > (unsigned int)kTailList) enqueue(q, cnt, rest, N);
  };
  auto block_flush = [&](u64* q, unsigned int* cnt) {
    __syncthreads();
    const unsigned int nl = s_nlist < (unsigned int)kTailList ? s_nlist : (unsigned int)kTailList;
    if (threadIdx.x == 0) s_nlong = 0;
    Index v[4], p[4];
    unsigned int pieces[4], mine = 0, mine_e = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned int at = threadIdx.x * 4 + i;
      v[i] = -1; p[i] = 0; pieces[i] = 0;
      if (at < nl) {
        v[i] = s_list[at];
        p[i] = a.optr[v[i]];
        const Index e = a.optr[v[i] + 1];
        pieces[i] = e > p[i] ? (unsigned int)((e - p[i] + kTailPiece - 1) / kTailPiece) : 1u;
        mine += pieces[i];
        mine_e += (unsigned int)(e - p[i]);
      }
    }
    unsigned int inc = mine, ince = mine_e;
inc = (unsigned int)wave_incl_scan_u32((unsigned)inc);
ince = (unsigned int)wave_incl_scan_u32((unsigned)ince);
    if (lane == kWave - 1) { s_wp[w] = inc; s_we[w] = ince; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned int tp = 0;
      unsigned long long te = 0;
      for (int i = 0; i < kPWaves; ++i) { const unsigned int x = s_wp[i]; s_wp[i] = tp; tp += x; te += s_we[i]; }
      s_base = 0; s_before = 0;
      if (tp) {
        s_base = atomicAdd(cnt, tp);
        s_before = atomicAdd((unsigned long long*)(cnt + 2), te);
      }
      s_nlist = 0;
    }
    __syncthreads();
    if (s_before <= t.edge_limit) {
      unsigned int at = s_base + s_wp[w] + inc - mine;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (pieces[i] > 8u) {
          const unsigned int li = atomicAdd(&s_nlong, 1u);
          if (li < (unsigned int)kTailLong) s_long[li] = make_int4(v[i], p[i], (int)pieces[i], (int)at);
          else
            for (unsigned int c = 0; c < pieces[i]; ++c)
              publish(&q[at + c], ((u64)(unsigned int)(p[i] + (Index)c * kTailPiece) << 32) | (u64)(unsigned int)(c == 0 ? v[i] : ~v[i]));
        } else {
          for (unsigned int c = 0; c < pieces[i]; ++c)
            publish(&q[at + c], ((u64)(unsigned int)(p[i] + (Index)c * kTailPiece) << 32) | (u64)(unsigned int)(c == 0 ? v[i] : ~v[i]));
        }
        at += pieces[i];
      }
      __syncthreads();
      const unsigned int nlong = s_nlong < (unsigned int)kTailLong ? s_nlong : (unsigned int)kTailLong;
      for (unsigned int li = 0; li < nlong; ++li) {
        const int4 L = s_long[li];
        for (unsigned int c = threadIdx.x; c < (unsigned int)L.z; c += kPThreads)
          publish(&q[(unsigned int)L.w + c], ((u64)(unsigned int)(L.y + (Index)c * kTailPiece) << 32) | (u64)(unsigned int)(c == 0 ? L.x : ~L.x));
      }
    }
    __syncthreads();
  };
  if (threadIdx.x == 0) s_nlist = 0;
  __syncthreads();

  {                                                         // the first queue: one pass over the stored frontier words, four chunks in flight
    const Index nchunks = (a.n + kWave - 1) / kWave;
    for (Index chunk = (Index)gw * 4; chunk < nchunks; chunk += (Index)nw * 4) {
      u64 fw[4];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const Index u = (chunk + r4) * kWave + lane;
        fw[r4] = u < a.n ? (t.f0[u] & a.pmask) : 0ull;
      }
      Index vq[4];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) vq[r4] = fw[r4] ? (chunk + r4) * kWave + lane : -1;
      collect(t.queue[0], &st->count[0][0], vq, 4);
    }
  }
  block_flush(t.queue[0], &st->count[0][0]);
  stamp();
  if (!grid_sync(&st->bar, gen)) return;
  stamp();

  int iter = t.iter0, j = 0, status = 0;
  unsigned long long levels = 0, cum_edges = 0, cum_pairs = 0;
  for (;;) {
    totals_init(&lds);
    WaveTotals tot;
    if (blockIdx.x == 0) {
      u64* z = st->slots[(j + 1) % 3];
      for (int i = threadIdx.x; i < kBatchSlots * kBatchCounters; i += kPThreads) publish(&z[i], 0ull);
      if (threadIdx.x < 4) publish(&st->count[(j + 2) & 3][threadIdx.x], 0u);   // length, and the out-edges behind it
      if (threadIdx.x < 16) publish(&st->dec[(j + 1) % 3][threadIdx.x >> 1][threadIdx.x & 1], 0ull);
    }
    if (j >= 2) {                                           // the words level j - 1 read: the array level j + 1 will write
      const unsigned int mq = fresh(&st->count[(j - 1) & 3][0]);
      const u64* qp = t.queue[(j - 1) % 3];
      u64* Xw = t.X[(j - 2) % 3];
      for (unsigned int i = gt; i < mq; i += nt) {
        const int x = (int)(unsigned int)qp[i];
        if (x >= 0) publish(&Xw[x], 0ull);
      }
    }
    const u64* F = j == 0 ? t.f0 : t.X[(j - 1) % 3];
    u64* Xn = t.X[j % 3];
    const u64* qc = t.queue[j % 3];
    u64* qn = t.queue[(j + 1) % 3];
    unsigned int* cn = &st->count[(j + 1) & 3][0];
    const unsigned int m = fresh(&st->count[j & 3][0]);
    const float lab = (float)(iter + 1);
    // a short queue is spread over the waves (a step is a chain of dependent memory round trips: 64 pieces in one
    // wave are 64 such chains one after the other, one piece in each of 64 waves is one)
    const unsigned int per = m >= (unsigned long long)nw * kWave ? (unsigned int)kWave : (m + nw - 1) / nw > 0 ? (m + nw - 1) / nw : 1u;
    for (unsigned int c = gw; (unsigned long long)c * per < m; c += nw) {
      const unsigned int idx = c * per + lane;
      const bool has = (unsigned int)lane < per && idx < m;
      const u64 ent = has ? qc[idx] : 0ull;
      const int x = (int)(unsigned int)ent;
      const Index u = x >= 0 ? x : ~x;
      Index p = (Index)(ent >> 32), e = p;
      u64 fw = 0;
      if (has) {
        const Index re = a.optr[u + 1];
        e = p + kTailPiece < re ? p + kTailPiece : re;
        fw = F[u] & a.pmask;
      }
      const Index d = e - p;
      Index inc = d;
inc = (Index)wave_incl_scan_u32((unsigned)inc);
      const Index total = __shfl(inc, kWave - 1, kWave);
      __builtin_amdgcn_wave_barrier();
      s_pre[w][lane] = inc - d;
      s_p[w][lane] = p;
      s_fw[w][lane] = fw;
      __builtin_amdgcn_wave_barrier();
      for (Index base = 0; base < total; base += 4 * kWave) {
        Index dst[4];
        u64 bits[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const Index at = base + r4 * kWave + lane;
          dst[r4] = -1; bits[r4] = 0ull;
          if (at < total) {
            int r = 0;                                     // the last piece whose first edge is <= at
#pragma unroll
            for (int step = kWave / 2; step > 0; step >>= 1)
              if (s_pre[w][r + step] <= at) r += step;
            dst[r4] = a.oind[s_p[w][r] + (at - s_pre[w][r])];
            bits[r4] = s_fw[w][r];
          }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) bits[r4] = dst[r4] >= 0 ? (bits[r4] & ~a.seen[dst[r4]]) : 0ull;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          if (bits[r4]) bits[r4] &= ~atomicOr(&a.seen[dst[r4]], bits[r4]);
        Index vq[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) vq[r4] = bits[r4] && atomicOr(&Xn[dst[r4]], bits[r4]) == 0ull ? dst[r4] : -1;
        collect(qn, cn, vq, 4);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) batch_commit_l(a, tot, bits[r4] ? dst[r4] : 0, bits[r4], true, lab, false);
      }
      __builtin_amdgcn_wave_barrier();
    }
    block_flush(qn, cn);
    stamp();
    totals_flush_to(st->slots[j % 3], &lds, tot);          // per source: read by workgroup 0 when the launch ends, by nobody else
    if (t.per_source)                                       // ... and summed over the levels (light levels: few sources, few pairs)
      for (int i = threadIdx.x; i < 128; i += kPThreads) {
        const u64 x = lds.v[2 + i];
        if (x) {
          atomicAdd(&st->cum[i], x);
          if (!(i & 1)) atomicMax(&st->last[i >> 1], (unsigned int)iter);
        }
      }
    if (threadIdx.x < kWave) {                             // what everybody needs: the level's pairs and their out-edges
      u64 np = lds.v[2 + 2 * lane], ne = lds.v[3 + 2 * lane];
      np = wave_sum_u64(np); ne = wave_sum_u64(ne);
      if (lane == 0 && np) {
        atomicAdd(&st->dec[j % 3][blockIdx.x & 7][0], np);
        atomicAdd(&st->dec[j % 3][blockIdx.x & 7][1], ne);
      }
    }
    stamp();
    if (!grid_sync(&st->bar, gen)) return;
    stamp();
    if (threadIdx.x < kWave) {
      u64 x = lane < 16 ? fresh(&st->dec[j % 3][lane >> 1][lane & 1]) : 0ull;
      x += __shfl_xor(x, 2, kWave); x += __shfl_xor(x, 4, kWave); x += __shfl_xor(x, 8, kWave);   // lane 0: pairs, lane 1: edges
      if (lane < 2) s_dec[lane] = x;
    }
    __syncthreads();
    const u64 pairs = s_dec[0], edges = s_dec[1];
    ++levels;
    cum_pairs += pairs;
    cum_edges += edges;
    if (pairs == 0) { status = 0; break; }
    if (iter >= t.max_niter) { status = 1; break; }
    if (edges > t.edge_limit) { status = 2; break; }
    ++iter;
    ++j;
    __syncthreads();                                        // s_sum / s_dec are rewritten next level
  }
  if (j >= 1) {                                             // the words the last level read: every array but the new frontier's is left all-zero
    const unsigned int mq = fresh(&st->count[j & 3][0]);
    const u64* qp = t.queue[j % 3];
    u64* Xw = t.X[(j - 1) % 3];
    for (unsigned int i = gt; i < mq; i += nt) {
      const int x = (int)(unsigned int)qp[i];
      if (x >= 0) publish(&Xw[x], 0ull);
    }
  }
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < kBatchCounters; i += kPThreads) s_sum[i] = 0ull;
    __syncthreads();
    for (int i = threadIdx.x; i < kBatchSlots * kBatchCounters; i += kPThreads) {
      const u64 x = fresh(&st->slots[j % 3][i]);
      if (x) atomicAdd(&s_sum[i % kBatchCounters], x);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBatchCounters; i += kPThreads)
      __hip_atomic_store(&t.box[i], s_sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) {
      __hip_atomic_store(&t.box[kBatchCounters + 1], (u64)levels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&t.box[kBatchCounters + 2], (u64)cum_edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&t.box[kBatchCounters + 3], (u64)cum_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&t.box[kBatchCounters + 4], (u64)status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      *t.status = (u64)status;
    }
    if (t.per_source)
      for (int i = threadIdx.x; i < 128 + 64; i += kPThreads)
        __hip_atomic_store(&t.box[kBatchBoxPer + i], i < 128 ? fresh(&st->cum[i]) : (u64)fresh(&st->last[i - 128]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&t.box[kBatchCounters], t.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void batch_unlabel_kernel(BatchArgs a, float bad) {
  for (int s = 0; s < a.k; ++s)
    for (Index i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x)
      if (a.label[s][i] == bad) a.label[s][i] = 0.f;
}

// ---- the hot block's preparation, once per matrix ----------------------------------------------------------------------
// The threshold is found by selecting the (cap + 1)-th largest out-degree digit by digit: a pass counts, in LDS, one
// 11-bit digit of the degrees that agree with the digits chosen so far (the host reads 2048 counts, never a degree).
constexpr int kHotDigitBits = 11, kHotBins = 1 << kHotDigitBits;
__global__ __launch_bounds__(kBlock) void batch_hot_hist_kernel(const Index* __restrict__ optr, Index n, unsigned int above_mask,
                                                                unsigned int above_value, int shift, unsigned int* __restrict__ bins) {
  __shared__ unsigned int s_bins[kHotBins];
  for (int i = threadIdx.x; i < kHotBins; i += blockDim.x) s_bins[i] = 0u;
  __syncthreads();
  for (Index v = (Index)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (Index)gridDim.x * blockDim.x) {
    const unsigned int d = (unsigned int)(optr[v + 1] - optr[v]);
    if ((d & above_mask) == above_value) atomicAdd(&s_bins[(d >> shift) & (unsigned int)(kHotBins - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHotBins; i += blockDim.x)
    if (s_bins[i]) atomicAdd(&bins[i], s_bins[i]);
}
// flag[v] = 1 for a hub, flag[n] = 0: scanned, flag[v] is the hub's slot and flag[n] is H
__global__ __launch_bounds__(kBlock) void batch_hot_flag_kernel(const Index* __restrict__ optr, Index n, unsigned int t,
                                                                unsigned int* __restrict__ flag) {
  for (Index v = (Index)blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += (Index)gridDim.x * blockDim.x)
    flag[v] = v < n && (unsigned int)(optr[v + 1] - optr[v]) >= t ? 1u : 0u;
}
// the scanned flags become the table old name -> new name, in place; the hubs are listed by slot
__global__ __launch_bounds__(kBlock) void batch_hot_names_kernel(const Index* __restrict__ optr, Index n, unsigned int t,
                                                                 unsigned int* __restrict__ slot_then_name, Index* __restrict__ hubs) {
  for (Index v = (Index)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (Index)gridDim.x * blockDim.x) {
    const bool hub = (unsigned int)(optr[v + 1] - optr[v]) >= t;
    const unsigned int j = slot_then_name[v];
    if (hub) hubs[j] = v;
    slot_then_name[v] = hub ? (unsigned int)n + j : (unsigned int)v;
  }
}
// out[i] = name[in[i]]; an entry that names no vertex (the hint of a row without entries: -1) stays
__global__ __launch_bounds__(kBlock) void batch_hot_rename_kernel(const Index* __restrict__ in, long long count, Index n,
                                                                  const unsigned int* __restrict__ name, Index* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
    const Index c = in[i];
    out[i] = c >= 0 && c < n ? (Index)name[c] : c;
  }
}

}  // namespace grb

using namespace grb;

// rows of >= kBatchBig entries cut into slices; cached per matrix and orientation
static int batch_big(bool in_edges) {
  static const int big_in = getenv("GRB_BATCH_BIG_IN") ? atoi(getenv("GRB_BATCH_BIG_IN")) : kBatchBig;
  static const int big_out = getenv("GRB_BATCH_BIG_OUT") ? atoi(getenv("GRB_BATCH_BIG_OUT")) : kBatchBigPush;
  const int b = in_edges ? big_in : big_out;
  return b < 64 ? 64 : b;
}

static grb_info make_slices(grb_matrix A, bool in_edges);
static grb_info ensure_slices(grb_matrix A, bool in_edges) {
  BatchSlices& B = in_edges ? A->batch_in : A->batch_out;
  if (B.ready) return GRB_SUCCESS;
  const grb_info i = make_slices(A, in_edges);
  if (i != GRB_SUCCESS) {                                   // nothing half-made stays behind
    (void)hipStreamSynchronize(ctx().stream);
    if (B.d_slices) (void)hipFree(B.d_slices);
    if (B.d_rows) (void)hipFree(B.d_rows);
    if (B.d_range_off) (void)hipFree(B.d_range_off);
    if (B.d_range_bounds) (void)hipFree(B.d_range_bounds);
    if (B.d_range_ids) (void)hipFree(B.d_range_ids);
    if (B.d_big_index) (void)hipFree(B.d_big_index);
    B = BatchSlices();
  }
  return i;
}
static grb_info make_slices(grb_matrix A, bool in_edges) {
  BatchSlices& B = in_edges ? A->batch_in : A->batch_out;
  const std::vector<Index>& ptr = in_edges ? A->h_csc_ptr : A->h_csr_ptr;
  const Index n = in_edges ? A->ncols : A->nrows;
  if ((Index)ptr.size() != n + 1) return GRB_INVALID_OBJECT;
  std::vector<int4> sl;
  std::vector<Index> rows;
  for (Index v = 0; v < n; ++v) {
    const Index d = ptr[(size_t)v + 1] - ptr[v];
    if (d < batch_big(in_edges)) continue;
    const Index step = std::min<Index>(batch_big(in_edges), in_edges ? kBatchSlice : kBatchPushSlice);
    for (Index s = ptr[v]; s < ptr[(size_t)v + 1]; s += step)
      sl.push_back(make_int4(v, s, std::min<Index>(s + step, ptr[(size_t)v + 1]), (int)rows.size()));
    rows.push_back(v);
  }
  B.nslices = (int)sl.size();
  B.nbig = (int)rows.size();
  if (B.nslices > 0) {
    GRB_HIP_TRY(hipMalloc((void**)&B.d_slices, sizeof(int4) * sl.size()));
    GRB_HIP_TRY(hipMalloc((void**)&B.d_rows, sizeof(Index) * rows.size()));
    GRB_HIP_TRY(hipMemcpy(B.d_slices, sl.data(), sizeof(int4) * sl.size(), hipMemcpyHostToDevice));
    GRB_HIP_TRY(hipMemcpy(B.d_rows, rows.data(), sizeof(Index) * rows.size(), hipMemcpyHostToDevice));
    // out-edges: where each big row enters each destination range (the owner-computes push of heavy levels); ranges of
    // equal in-degree mass, about four per CU-sized share, at most kOwnRows rows
    if (!in_edges && n >= 2 * kOwnRows) {
      const std::vector<Index>& iptr = (Index)A->h_csc_ptr.size() == n + 1 ? A->h_csc_ptr : A->h_csr_ptr;
      const long long total = (long long)iptr[(size_t)n];
      const long long target = std::max<long long>(1, total / (3 * 256));
      std::vector<Index> bounds(1, 0);
      while (bounds.back() < n) {
        const Index s0 = bounds.back();
        Index e = (Index)std::min<long long>((long long)n, (long long)s0 + kOwnRows);
        // the last row whose prefix stays within the target, at least one row
        const Index* lo = iptr.data() + s0 + 1;
        const Index* hi = iptr.data() + e + 1;
        const Index* cut = std::upper_bound(lo, hi, (Index)std::min<long long>((long long)iptr[s0] + target, 0x7fffffffll));
        Index e2 = (Index)(cut - iptr.data()) - 1;
        if (e2 <= s0) e2 = s0 + 1;
        if (e2 < e) e = e2;
        bounds.push_back(e);
      }
      const long long R = (long long)bounds.size() - 1;
      const long long S = own_off_stride(R);                 // the table's row stride: whole 128-byte lines
      if (R >= 2 && (long long)rows.size() * S <= (128ll << 20)) {
        GRB_HIP_TRY(hipMalloc((void**)&B.d_range_bounds, sizeof(Index) * bounds.size()));
        GRB_HIP_TRY(hipMemcpy(B.d_range_bounds, bounds.data(), sizeof(Index) * bounds.size(), hipMemcpyHostToDevice));
        GRB_HIP_TRY(hipMalloc((void**)&B.d_range_off, sizeof(Index) * rows.size() * (size_t)S));
        hipLaunchKernelGGL(batch_range_off_kernel, dim3(stream_grid((long long)rows.size() * (R + 1), kBlock)), dim3(kBlock), 0,
                           ctx().stream, A->csr.ptr, A->csr.ind, B.d_rows, (int)rows.size(), (int)R, (int)S,
                           (const Index*)B.d_range_bounds, B.d_range_off);
        GRB_HIP_TRY(hipGetLastError());
        B.nranges = (int)R;
        std::vector<int> ids;
        // Within an instantiation, workgroup p runs on XCD p % 8 (round-robin dispatch): the ranges are dealt so that each
        // XCD gets a contiguous eighth of them, and the 32 ranges that share a line of the offsets table share an L2.
        for (int pass = 0; pass < 2; ++pass) {
          std::vector<int> mine;
          for (long long b = 0; b < R; ++b)
            if ((bounds[(size_t)b + 1] - bounds[(size_t)b] <= kOwnSmallRows) == (pass == 0)) mine.push_back((int)b);
          const size_t m = mine.size(), q = m / 8, r = m % 8;
          for (size_t j = 0; j <= q; ++j)
            for (size_t x = 0; x < 8; ++x)
              if (j < q + (x < r ? 1 : 0)) ids.push_back(mine[x * q + std::min(x, r) + j]);
          if (pass == 0) B.nsmall = (int)ids.size();
        }
        GRB_HIP_TRY(hipMalloc((void**)&B.d_range_ids, sizeof(int) * ids.size()));
        GRB_HIP_TRY(hipMemcpy(B.d_range_ids, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice));
        // vertex -> big index: batch_push_kernel lists the big frontier rows it skips by it (read for big rows only)
        std::vector<int> big_index((size_t)n, -1);
        for (size_t bi = 0; bi < rows.size(); ++bi) big_index[(size_t)rows[bi]] = (int)bi;
        GRB_HIP_TRY(hipMalloc((void**)&B.d_big_index, sizeof(int) * (size_t)n));
        GRB_HIP_TRY(hipMemcpy(B.d_big_index, big_index.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
      }
    }
  }
  B.ready = true;
  return GRB_SUCCESS;
}

// ---- the hot block, per matrix (kernels and the why: batch_totals_kernel's neighbours above) -------------------------------
// At most this many hubs (GRB_BATCH_HOT_MAX; GRB_BATCH_HOT=0: none).  Read once per process.
constexpr long long kBatchHotMax = 64 << 10;
static long long batch_hot_cap() {
  static const long long cap = [] {
    const char* on = getenv("GRB_BATCH_HOT");
    if (on && atoi(on) == 0) return 0ll;
    const char* e = getenv("GRB_BATCH_HOT_MAX");
    const long long c = e ? atoll(e) : kBatchHotMax;
    return c < 0 ? 0ll : c;
  }();
  return cap;
}
static void hot_drop(grb_matrix A) {                        // the matrix sweeps without a hot block from here on
  BatchHot& B = A->batch_hot;
  (void)hipStreamSynchronize(ctx().stream);
  if (B.d_hubs) (void)hipFree(B.d_hubs);
  if (B.d_iind) (void)hipFree(B.d_iind);
  if (B.d_hint) (void)hipFree(B.d_hint);
  B.d_hubs = B.d_iind = B.d_hint = nullptr;
  B.H = 0;
}
// what make_hot may allocate for at most Hb hubs, scratch included
static size_t hot_bound(grb_matrix A, long long Hb) {
  const size_t n = (size_t)A->nrows;
  return 4 * ((size_t)A->nvals + 1) + 4 * n + 4 * (n + 1) + 256 + device_scan_u32_scratch((long long)n + 1) + 4 * (size_t)Hb + 4 * kHotBins + 4096;
}
namespace {
struct HotScratch {
  void* p = nullptr;
  ~HotScratch() { if (p) (void)hipFree(p); }
};
}  // namespace
static grb_info make_hot(grb_matrix A) {
  BatchHot& B = A->batch_hot;
  hipStream_t st = ctx().stream;
  const Index n = A->nrows;
  const Index* optr = A->csr.ptr;
  // t: one more than the (cap + 1)-th largest out-degree -- the smallest threshold that leaves at most cap vertices.  Ties
  // at that degree stay out together, so the hubs do not depend on any order among equals.
  long long H = n;
  B.t = 0;
  if (B.cap < (long long)n) {
    HotScratch bins_d;
    GRB_HIP_TRY(hipMalloc(&bins_d.p, sizeof(unsigned int) * kHotBins));
    std::vector<unsigned int> bins(kHotBins);
    unsigned int mask = 0, value = 0;
    long long rank = B.cap;                                 // of the degree looked for, from the largest, among the degrees that agree with `value` on `mask`
    for (int shift = 2 * kHotDigitBits; shift >= 0; shift -= kHotDigitBits) {
      GRB_HIP_TRY(hipMemsetAsync(bins_d.p, 0, sizeof(unsigned int) * kHotBins, st));
      hipLaunchKernelGGL(batch_hot_hist_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, optr, n, mask, value, shift, (unsigned int*)bins_d.p);
      GRB_HIP_TRY(hipGetLastError());
      GRB_HIP_TRY(hipMemcpyAsync(bins.data(), bins_d.p, sizeof(unsigned int) * kHotBins, hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipStreamSynchronize(st));
      int digit = kHotBins - 1;
      for (; digit > 0 && rank >= (long long)bins[digit]; --digit) rank -= (long long)bins[digit];
      if (rank >= (long long)bins[digit]) return GRB_PANIC;  // (more than cap degrees were counted: the digit is among them)
      value |= (unsigned int)digit << shift;
      mask |= (unsigned int)(kHotBins - 1) << shift;
    }
    B.t = (long long)value + 1;
    H = B.cap - rank;                                       // the degrees above the one selected
  }
  if (H <= 0 || B.t > 0x7fffffffll) return GRB_SUCCESS;
  if ((long long)n + H > 0x7fffffffll - 64) return GRB_SUCCESS;   // a renamed index is n + slot, an Index
  HotScratch names;
  const size_t flag_bytes = (sizeof(unsigned int) * ((size_t)n + 1) + 255) & ~(size_t)255;
  GRB_HIP_TRY(hipMalloc(&names.p, flag_bytes + device_scan_u32_scratch((long long)n + 1)));
  unsigned int* const d_name = (unsigned int*)names.p;
  hipLaunchKernelGGL(batch_hot_flag_kernel, dim3(stream_grid((long long)n + 1, kBlock)), dim3(kBlock), 0, st, optr, n, (unsigned int)B.t, d_name);
  GRB_HIP_TRY(hipGetLastError());
  GRB_TRY(device_exclusive_scan_u32_in(d_name, (long long)n + 1, (unsigned int*)((char*)names.p + flag_bytes)));
  unsigned int counted = 0;
  GRB_HIP_TRY(hipMemcpyAsync(&counted, d_name + n, sizeof(counted), hipMemcpyDeviceToHost, st));
  GRB_HIP_TRY(hipStreamSynchronize(st));
  if ((long long)counted != H) return GRB_PANIC;
  GRB_HIP_TRY(hipMalloc((void**)&B.d_hubs, sizeof(Index) * (size_t)H));
  GRB_HIP_TRY(hipMalloc((void**)&B.d_iind, sizeof(Index) * ((size_t)A->nvals + 1)));
  GRB_HIP_TRY(hipMalloc((void**)&B.d_hint, sizeof(Index) * (size_t)n));
  hipLaunchKernelGGL(batch_hot_names_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, optr, n, (unsigned int)B.t, d_name, B.d_hubs);
  if (A->nvals > 0)
    hipLaunchKernelGGL(batch_hot_rename_kernel, dim3(stream_grid(A->nvals, kBlock)), dim3(kBlock), 0, st, (const Index*)A->csc.ind,
                       (long long)A->nvals, n, (const unsigned int*)d_name, B.d_iind);
  hipLaunchKernelGGL(batch_hot_rename_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, (const Index*)A->d_pull_hint, (long long)n, n,
                     (const unsigned int*)d_name, B.d_hint);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipStreamSynchronize(st));                    // (the name table goes when this returns)
  B.H = (Index)H;
  return GRB_SUCCESS;
}
// With the pull hint and before the sweep's sizes are taken.  Never an error: whatever stops it -- an allocation included --
// leaves H = 0, and the matrix sweeps as it did without a hot block.  allowed = false: the caller's memory rule said no.
static void ensure_hot(grb_matrix A, bool allowed = true) {
  BatchHot& B = A->batch_hot;
  if (B.ready) return;
  B = BatchHot();
  B.ready = true;
  B.cap = batch_hot_cap();
  const bool can = allowed && B.cap > 0 && A->format == 0 && !A->csc_alias && A->nrows >= 1 && A->d_pull_hint && A->csr.ptr && A->csc.ind;
  if (can && make_hot(A) != GRB_SUCCESS) {
    (void)hipGetLastError();
    hot_drop(A);
  }
  if (getenv("GRB_BATCH_TRACE"))
    fprintf(stderr, "sweep hot block: H %d, t %lld, cap %lld%s\n", (int)B.H, B.t, B.cap, allowed ? "" : " (no memory for it)");
}

extern "C" grb_info grb_bfs_batch_hot(grb_matrix A, long long* H, long long* t, long long* cap, grb_index* hubs, long long hubs_len) { GRB_API_ENTER();
  if (!A) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built || !A->csr.ptr || !A->csc.ptr) return GRB_UNINITIALIZED_OBJECT;
  if (A->nrows != A->ncols) return GRB_DIMENSION_MISMATCH;
  GRB_TRY(ctx_init());
  GRB_TRY(ensure_pull_hint(&A->d_pull_hint, A->csc, A->csr.ptr, ctx().stream));
  ensure_hot(A);
  const BatchHot& B = A->batch_hot;
  if (H) *H = B.H;
  if (t) *t = B.t;
  if (cap) *cap = B.cap;
  const long long m = std::min<long long>(B.H, hubs_len);
  if (hubs && m > 0) GRB_HIP_TRY(hipMemcpy(hubs, B.d_hubs, sizeof(Index) * (size_t)m, hipMemcpyDeviceToHost));
  return GRB_SUCCESS;
}

// out-edges a level may push inside the light-level launch (0: every level through the host loop)
static long long& batch_tail_limit() {
  static long long limit = [] {
    const char* on = getenv("GRB_BATCH_TAIL");
    if (on && atoi(on) == 0) return 0ll;
    const char* e = getenv("GRB_BATCH_TAIL_EDGES");
    return e ? atoll(e) : 1048576ll;
  }();
  return limit;
}

extern "C" long long grb_bfs_batch_set_tail(long long edges) { GRB_API_ENTER_NOINFO();
  const long long before = batch_tail_limit();
  if (edges >= 0) batch_tail_limit() = edges;
  return before;
}

// ---- the sweep proper ------------------------------------------------------------------------------------------------
// What the sweep keeps between its kernels.  grb_bfs_batch runs on the library's scratch slots (own == nullptr); the
// sweep the traversal queue routes its gathered groups to (bfs_persist.hip) runs on buffers of its own, provisioned
// once (bfs_sweep_provision) -- slot 7 is the one-launch traversal's pre-zeroed block, and a blocking call after a routed
// sweep must not find it taken.
namespace {
// The rotating word arrays a complete sweep left all-zero, and the sizes it ran at (the light-level launch leaves its
// arrays so).  take() hands the knowledge to the sweep that starts and voids the record: a sweep that fails in between
// leaves none.
struct SweepClean {
  bool valid = false, clean[4] = {false, false, false, false};
  Index n = 0;
  size_t stride = 0;
  int nstore = 0;
  void take(bool mine, Index n_, size_t stride_, int nstore_, bool* out) {
    const bool ok = mine && valid && n == n_ && stride == stride_ && nstore == nstore_;
    for (int i = 0; i < 4; ++i) out[i] = ok && clean[i];
    valid = false;
  }
  void keep(Index n_, size_t stride_, int nstore_, const bool* now) {
    valid = true; n = n_; stride = stride_; nstore = nstore_;
    for (int i = 0; i < 4; ++i) clean[i] = now[i];
  }
};
struct SweepOwn {
  void *words = nullptr, *cnt = nullptr, *tail = nullptr, *list = nullptr;
  size_t words_cap = 0, tail_cap = 0, list_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  SweepClean zero;                                          // (nobody else ever has these buffers)
  bool small_clean = false;                                 // the counter slots and the big-row list's length are zero, as every complete sweep leaves them
  bool warmed = false;                                      // every batch_* kernel has been launched once ...
  bool warmed_own_small = false, warmed_own_wide = false;   // ... the two owner-computes instances too (they need a matrix with ranges)
};
SweepOwn g_sweep;
// the scratch-slot route's events and its record, which holds only while nobody else has had slot 7 in between
struct SweepScratch {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  SweepClean zero;
  unsigned long long epoch = 0;
  void* ptr = nullptr;
};
SweepScratch g_sweep_scratch;
struct SweepSizes {
  int nstore = 1;
  size_t stride = 0;                                        // words from one array to the next: n, or n + H rounded up to 256 bytes
  size_t words = 0, tail = 0, tail_state = 0, qcap = 0, list = 0, list_ids = 0;
};
struct SweepTotals {                                        // the whole sweep's, as grb_bfs_batch reports them
  int levels = 0, last_dir = 0;
  unsigned long long edges = 0, reached = 0;
  bool hit_cap = false;
  float ms = 0.f;
};
u64 *g_box_h = nullptr, *g_box_d = nullptr;                 // {totals, sequence number, ...}: pinned, host-coherent
u64 g_box_seq = 0;
}  // namespace

// (H: the hot block's hubs -- the matrix's own, or a bound on them before they are known)
static SweepSizes sweep_sizes(grb_matrix A, long long H) {
  SweepSizes z;
  const Index n = A->nrows;
  // every array a pull can read as its frontier carries the hubs' words behind its n; seen is spaced like the rest
  z.stride = H > 0 ? (((size_t)n + (size_t)H + 31) & ~(size_t)31) : (size_t)n;
  // stored level words: as many as fit 1 GiB, at most kBatchStoreMax (+ the seed words) + two rotating buffers
  z.nstore = (int)((1ull << 30) / (sizeof(u64) * (z.stride > 0 ? z.stride : 1)));
  if (z.nstore > kBatchStoreMax) z.nstore = kBatchStoreMax;
  if (z.nstore < 1) z.nstore = 1;
  const int nbuf = 1 + (z.nstore + 1) + 4;                  // seen, the kept levels' words, four rotating arrays
  z.words = (size_t)nbuf * sizeof(u64) * z.stride + 256;
  z.qcap = (size_t)n + (size_t)(A->nvals / kTailPiece) + 64;
  z.tail_state = (sizeof(TailState) + 255) & ~(size_t)255;
  z.tail = kTailStates * z.tail_state + 3 * sizeof(u64) * z.qcap;
  z.list_ids = (sizeof(int) * (size_t)kListSegs * (size_t)A->batch_out.nbig + 255) & ~(size_t)255;
  z.list = kListHeader + z.list_ids + sizeof(u64) * (size_t)kListSegs * (size_t)A->batch_out.nbig;
  return z;
}
static SweepSizes sweep_sizes(grb_matrix A) { return sweep_sizes(A, A->batch_hot.H); }

static grb_info batch_box() {
  if (g_box_h) return GRB_SUCCESS;
  GRB_HIP_TRY(hipHostMalloc((void**)&g_box_h, sizeof(u64) * kBatchBoxWords, hipHostMallocMapped | hipHostMallocCoherent));
  memset(g_box_h, 0, sizeof(u64) * kBatchBoxWords);
  GRB_HIP_TRY(hipHostGetDevicePointer((void**)&g_box_d, g_box_h, 0));
  return GRB_SUCCESS;
}

// ---- layouts and launch sites the sweep shares with sweep_warm ---------------------------------------------------------
namespace {
struct ListBlock {                                          // the big-row list of an owner-computes level
  unsigned int* len;                                        // kListSegs lengths, kListLenStride apart
  int* ids;
  u64* words;
};
}  // namespace
static ListBlock list_carve(void* p_list, const SweepSizes& z) {
  return {(unsigned int*)p_list, (int*)((char*)p_list + kListHeader), (u64*)((char*)p_list + kListHeader + z.list_ids)};
}
// the light-level launch's state block `state` of the kTailStates and its three queues behind them
static void tail_carve(TailArgs& t, void* p_tail, const SweepSizes& z, int state) {
  t.st = (TailState*)((char*)p_tail + (size_t)state * z.tail_state);
  for (int i = 0; i < 3; ++i) t.queue[i] = (u64*)((char*)p_tail + kTailStates * z.tail_state) + (size_t)i * z.qcap;
}
// the owners of `count` destination ranges, taken from range_ids[first] on
template <int Rows, int Threads>
static void launch_owners(const BatchArgs& a, const BatchSlices& B, const ListBlock& L, int first, int count, hipStream_t st) {
  hipLaunchKernelGGL((batch_push_owner_kernel<Rows, Threads>), dim3(count), dim3(Threads), 0, st, a, (const Index*)B.d_range_off,
                     (int)own_off_stride(B.nranges), (const int*)L.ids, (const u64*)L.words, (const unsigned int*)L.len,
                     (const Index*)B.d_range_bounds, (const int*)B.d_range_ids + first);
}

// ---- the knobs, read at the first sweep of the process ------------------------------------------------------------------
namespace {
struct SweepKnobs {
  bool trace;                                               // GRB_BATCH_TRACE: a line per level on stderr
  // ---- direction per source: the reference's vertex-count rule (switchpoint) on that source's own frontier, and a
  // budget on the edges pushed in one level (batch_decide.hpp): pull the sources whose own frontier passed the
  // reference's switch point (their bits are found within a few probes, so the early exit works); push the others --
  // unless their out-edges together exceed 0.15 of the matrix (GRB_BATCH_BUDGET: a pushed edge is a random line of seen
  // plus an atomic on it, about 50 G edges/s on RMAT-22 against 85 G/s for a pulled entry), then the heaviest of them
  // are pulled as well.  The host decides the sweep's first level and the one after a light-level launch; after a level
  // of this loop the totals kernel has decided the next one on the device, and that decision is the one used.
  double budget;
  // ---- the finishing rule.  At a sweep's end a source is under the switch point because almost nothing is left for it to
  // find, and pushing it costs what a push stage costs whatever it pushes: batch_push_kernel reads all n frontier words to
  // find the few that carry a pushed bit, batch_push_commit_kernel reads all n words again to count what arrived (26 us a
  // level on RMAT-22, 41 with the slice kernel, for 60-125 K edges) -- while the same level pulls other sources over all n
  // rows anyway.  The pull kernels count U, the in-edges of the rows they leave open (counter kCntOpenU): after a level
  // that pulled every live source U bounds what the next pull can inspect, for all sources.  When the per-source rule
  // would pull some sources and push others and U <= finish_limit * nvals (GRB_BATCH_FINISH_LIMIT, 0.01), the pushed
  // sources are pulled too and the level has no push stage (batch_decide_finish).  Only the totals kernel ever has a
  // complete U: the levels the host decides (the first, the one after a light-level launch) keep the per-source rule, as
  // does a level after one that pushed anything or a level that pulls nobody.  GRB_BATCH_FINISH=0: no such rule.
  double finish_limit;
  // Launching ahead: behind a level's totals kernel the NEXT level's pull kernels are enqueued at once, before the host
  // has the totals -- they take their bits from the control block the totals kernel leaves, and return at once when that
  // level is no level of this loop.  The GPU then pulls while the host turns the level round.  Stream order is all this
  // relies on.  GRB_BATCH_AHEAD=0: wait, then launch (for A/B runs in fresh processes).
  bool ahead;
  bool owner;                                               // GRB_BATCH_OWNER=0: no owner-computes push, the slice kernel takes the big rows
  bool owner_merge;                                         // GRB_BATCH_OWNER_MERGE=0: always the two owner launches (push_stage)
};
}  // namespace
static const SweepKnobs& sweep_knobs() {
  static const SweepKnobs knobs = [] {
    auto on = [](const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; };
    SweepKnobs x;
    x.trace = getenv("GRB_BATCH_TRACE") != nullptr;
    x.budget = getenv("GRB_BATCH_BUDGET") ? atof(getenv("GRB_BATCH_BUDGET")) : 0.15;
    const char* limit = getenv("GRB_BATCH_FINISH_LIMIT");
    x.finish_limit = !on("GRB_BATCH_FINISH") ? -1.0 : limit ? atof(limit) : 0.01;
    x.ahead = on("GRB_BATCH_AHEAD");
    x.owner = on("GRB_BATCH_OWNER");
    x.owner_merge = on("GRB_BATCH_OWNER_MERGE");
    return x;
  }();
  return knobs;
}

// ---- where the sweep's four buffers, two events and its record of zero arrays come from ---------------------------------
namespace {
struct SweepBufs {
  void *words = nullptr, *cnt = nullptr, *tail = nullptr, *list = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  SweepClean* zero = nullptr;
  bool zero_mine = false;                                   // nobody else has had the words since the record was made
};
}  // namespace
// own: the provisioned buffers.  Else scratch slots 7, 10, 11 and (with_tail) 8 -- and when slot 7 has no room for the
// hubs' tails the matrix loses its hot block and z is taken again.
static grb_info sweep_resolve(grb_matrix A, SweepOwn* own, bool with_tail, SweepSizes& z, SweepBufs& b) {
  if (own) {
    if (!own->words || own->words_cap < z.words || own->tail_cap < z.tail || own->list_cap < z.list || !own->ev0) return GRB_OUT_OF_MEMORY;
    b.words = own->words; b.cnt = own->cnt; b.tail = own->tail; b.list = own->list;
    b.ev0 = own->ev0; b.ev1 = own->ev1;
    b.zero = &own->zero;
    b.zero_mine = true;
    return GRB_SUCCESS;
  }
  Context& c = ctx();
  SweepScratch& s = g_sweep_scratch;
  grb_info wi = scratch(7, z.words, &b.words);
  if (wi != GRB_SUCCESS && A->batch_hot.H > 0) {            // no room for the tails: the sweep runs without the hot block
    (void)hipGetLastError();
    hot_drop(A);
    z = sweep_sizes(A);
    wi = scratch(7, z.words, &b.words);
  }
  GRB_TRY(wi);
  c.bfs_prezero_ptr = nullptr;                              // slot 7 is the one-launch traversal's pre-zeroed block
  GRB_TRY(scratch(10, sizeof(u64) * (kBatchSlots * kBatchCounters + kBatchCtlWords), &b.cnt));
  GRB_TRY(scratch(11, z.list, &b.list));
  if (with_tail) GRB_TRY(scratch(8, z.tail, &b.tail));
  if (!s.ev0) {
    GRB_HIP_TRY(hipEventCreate(&s.ev0));
    GRB_HIP_TRY(hipEventCreate(&s.ev1));
  }
  b.ev0 = s.ev0; b.ev1 = s.ev1;
  b.zero = &s.zero;
  b.zero_mine = s.epoch + 1 == c.slot_epoch[7] && s.ptr == b.words;
  return GRB_SUCCESS;
}

// ---- one sweep: what its stages share, and the stages in the order batch_sweep runs them --------------------------------
namespace {
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Sweep {
  // the call
  const int k;
  const grb_matrix A;
  const int max_niter;
  SweepOwn* const own;
  grb_bfs_result* const per;
  // fixed from begin() on
  const SweepKnobs& knobs = sweep_knobs();
  Context& c = ctx();
  const hipStream_t st = c.stream;
  const Index n = A->nrows;
  SweepSizes z = sweep_sizes(A);
  SweepBufs buf;
  ListBlock list;
  Index H = 0, Hcopy = 0;                                   // the hot block's hubs; those a totals launch copies (0 when nobody pulls: no tail is ever read)
  u64 *seen = nullptr, *d_ctl = nullptr;
  int grid = 0;
  double tail_edges = 0;
  bool ahead = false, first_plain = false;
  SeedSources seeds;
  BatchRule rule;
  BatchArgs a;
  BatchSlots slots;
  // the traversals so far
  unsigned long long nf_s[64], mf_s[64];                    // per-source frontier totals of the last level
  unsigned long long edges = 0, reached = 0;
  unsigned long long reached_s[64], edges_s[64];            // per source, for `per`
  int last_prod[64], dir_s[64];                             // the last iteration at which the source discovered anything; its direction
  int iter = 1, levels = 0, last_dir = 0;
  bool any_left = true;
  bool in_done = false;                                     // every big in-row has every source's bit: nothing left for the slice kernels
  // the tail of the frontier's array holds the hubs' words as they stand: a totals launch has copied them.  Not so for the
  // seeds' words, nor for the array a light-level launch hands back: a pull of those is preceded by a copy launch of its own
  bool tail_fresh = false;
  long long big_out_new = -1;                               // big out-rows among the frontier's vertices (-1: not counted, the light-level launch's hand-back)
  int tail_states_used = 0, light_status = 0;
  bool labels_done = false;                                 // the label pass behind the closing light-level launch has written the vectors
  // the level in hand
  double t_lvl = 0;
  BatchDecision dec;
  bool have_dec = false;
  u64 P = 0, Q = 0;
  double pushed_edges = 0;
  bool plain_level = false, heavy = false;
  bool pulled_ahead = false;                                // its pull kernels went out behind the totals kernel of the level before, by `planned`
  SlotPlan planned = {false, -1};

  Sweep(int k_, grb_matrix A_, int max_niter_, SweepOwn* own_, grb_bfs_result* per_) : k(k_), A(A_), max_niter(max_niter_), own(own_), per(per_) {}

  // level words: slot 0 .. nstore are kept for the label pass, four more rotate (batch_slots.hpp)
  u64* words(int slot) const { return slot < 0 ? nullptr : seen + (size_t)(1 + slot) * z.stride; }

  // results come back through the pinned, host-coherent box the host polls: no copy, no stream wait
  grb_info wait_box() {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (__atomic_load_n(&g_box_h[kBatchCounters], __ATOMIC_ACQUIRE) != g_box_seq) {
      if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) {
        GRB_HIP_TRY(hipStreamSynchronize(st));               // a long level, or a fault this wait reports
        if (__atomic_load_n(&g_box_h[kBatchCounters], __ATOMIC_ACQUIRE) != g_box_seq) return GRB_PANIC;
      }
    }
    return GRB_SUCCESS;
  }

  grb_info launch_pull(BatchArgs& x) {
    const BatchSlices& B = A->batch_in;
    x.big = in_done ? INT_MAX : batch_big(true);
    x.slices = B.d_slices; x.nslices = B.nslices; x.bigrows = B.d_rows; x.nbig = B.nbig;
    BatchArgs g = x;                                        // the two kernels that gather frontier words: hub j is n + j to them
    if (H > 0) { g.iind = A->batch_hot.d_iind; g.hint = A->batch_hot.d_hint; }
    hipLaunchKernelGGL(batch_pull_kernel, dim3(grid), dim3(kBlock), 0, st, g);
    GRB_HIP_TRY(hipGetLastError());
    if (B.nslices > 0 && !in_done) {
      hipLaunchKernelGGL(batch_pull_slices_kernel, dim3(stream_grid((long long)B.nslices * kWave, kBlock)), dim3(kBlock),
                         0, st, g);
      GRB_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(batch_big_apply_kernel, dim3(stream_grid(B.nbig, kBlock)), dim3(kBlock), 0, st, x);
      GRB_HIP_TRY(hipGetLastError());
    }
    return GRB_SUCCESS;
  }

  // the depth vectors from the kept levels as they stand; go != nullptr: only if that status word says the sweep is over
  grb_info launch_labels(const u64* go) {
    LabelArgs L;
    L.n = n; L.k = k;
    L.nstored = slots.nkept();
    L.seen = seen;
    L.go = go;
    for (int i = 0; i <= kBatchStoreMax; ++i) {
      const bool kept = i < slots.nkept();
      L.W[i] = kept ? words(i) : nullptr;
      // discovered by the last allowed iteration: never assigned (bfs.hpp:48-66)
      L.lab[i] = kept && slots.kept_level(i) + 1 <= max_niter ? (float)(slots.kept_level(i) + 1) : 0.f;
    }
    for (int s = 0; s < 64; ++s) L.label[s] = a.label[s];
    hipLaunchKernelGGL(batch_labels_kernel, dim3(grid), dim3(kBlock), 0, st, L);
    GRB_HIP_TRY(hipGetLastError());
    return GRB_SUCCESS;
  }

  grb_info begin(grb_vector* v, const grb_index* sources, int rules_mode, float switchpoint);
  bool decide();
  grb_info light_launch();
  grb_info pull_stage();
  grb_info push_stage();
  grb_info totals_and_ahead();
  grb_info read_level();
  grb_info finish(int* per_dir, SweepTotals* out);
};
}  // namespace

// buffers, the fills, the seed totals, the rule with the first level's decision, the seed kernel
grb_info Sweep::begin(grb_vector* v, const grb_index* sources, int rules_mode, float switchpoint) {
  tail_edges = (double)batch_tail_limit();
  const bool tail_on = tail_edges > 0;
  GRB_TRY(sweep_resolve(A, own, tail_on, z, buf));
  // the hot block: H hub words behind the n of every level-word array; the pull kernels' own copies of the CSC indices and
  // of the hint name hub j as n + j (H = 0: the matrix's arrays as they are)
  H = A->batch_hot.H;
  seen = (u64*)buf.words;
  list = list_carve(buf.list, z);
  bool clean[4];
  buf.zero->take(buf.zero_mine, n, z.stride, z.nstore, clean);
  slots.begin(z.nstore, clean);
  a.optr = A->csr.ptr; a.oind = A->csr.ind; a.iptr = A->csc.ptr; a.iind = A->csc.ind;
  a.hint = A->d_pull_hint;
  a.n = n;
  a.seen = seen;
  a.counters = (u64*)buf.cnt;
  a.k = k;
  a.ctl = nullptr;
  a.list_len = nullptr;
  a.claims = 0; a.stash = 0;
  a.big_index = nullptr; a.list = nullptr; a.list_fw = nullptr;
  a.big_out = batch_big(false);
  d_ctl = a.counters + kBatchSlots * kBatchCounters;        // written by every totals kernel before anybody reads it
  for (int s = 0; s < 64; ++s) a.label[s] = nullptr;
  for (int s = 0; s < k; ++s) {
    GRB_TRY(grb_vector_set_storage(v[s], GRB_DENSE));
    a.label[s] = (float*)v[s]->d_val;
  }
  GRB_TRY(batch_box());
  // The counter slots are left zero by every totals kernel and the big-row list's length by the commit kernel behind the
  // owner kernels, so a sweep that ran to its end leaves both zero; on the sweep's own buffers, which nobody else has, that
  // is remembered, and a sweep that fails in between clears them at the next start.
  if (!(own && own->small_clean)) {
    GRB_HIP_TRY(hipMemsetAsync(a.counters, 0, sizeof(u64) * kBatchSlots * kBatchCounters, st));
    GRB_HIP_TRY(hipMemsetAsync(list.len, 0, kListHeader, st));
  }
  if (own) own->small_clean = false;
  // the light-level launches' state blocks, all of them now: the fill runs while the host is still enqueuing the sweep's
  // start, not between a level's totals and the launch that waits for it
  if (tail_on) GRB_HIP_TRY(hipMemsetAsync(buf.tail, 0, kTailStates * z.tail_state, st));
  GRB_HIP_TRY(hipMemsetAsync(seen, 0, sizeof(u64) * (z.stride + (size_t)n), st));   // seen and the seeds' words (and seen's unused tail)
  for (int s = 0; s < 64; ++s) seeds.v[s] = s < k ? (Index)sources[s] : 0;
  reached = (unsigned long long)k;
  for (int s = 0; s < k; ++s) {
    nf_s[s] = 1;
    mf_s[s] = (unsigned long long)(A->h_csr_ptr[(size_t)sources[s] + 1] - A->h_csr_ptr[sources[s]]);
    edges += mf_s[s];
    reached_s[s] = 1; edges_s[s] = mf_s[s]; last_prod[s] = 0; dir_s[s] = 0;
  }
  // GRB_SPARSE_MATRIX_FORMAT = 1: no CSC storage -- the "CSC" arrays ARE the CSR arrays, and the reference's vxm
  // is forced to push whatever the mxvmode says (operations.hpp:131-133).  A pull over them would walk out-edges
  // as if they were in-edges: every source is pushed.
  const int mode = (A->format != 0 || A->csc_alias) ? GRB_PUSHONLY : rules_mode;
  grid = stream_grid((long long)ceil_div(n, kWave) * kWave, kBlock);
  rule.k = k; rule.n = (long long)n; rule.nvals = (long long)A->nvals;
  rule.mode = mode == GRB_PULLONLY ? kDecidePullOnly : mode == GRB_PUSHONLY ? kDecidePushOnly : kDecidePushPull;
  rule.switchpoint = switchpoint; rule.budget = knobs.budget; rule.tail_limit = tail_on ? tail_edges : 0.0;
  rule.finish_limit = knobs.finish_limit;
  ahead = knobs.ahead && mode != GRB_PUSHONLY;
  Hcopy = mode == GRB_PUSHONLY ? 0 : H;
  // The first level: when the rule pushes every source (light or not), it runs as a host level whose push is
  // batch_first_level_kernel.  The seeds then need no words of their own -- their labels are written by the seed kernel,
  // directly -- and slot 0 takes the level's words.  Any source pulled (pull-only rules, a switch point at 0, sources over
  // the budget): the seeds are a stored level and the level runs through the general kernels.
  if (max_niter >= 1) {
    dec = batch_decide(nf_s, mf_s, rule, true);
    have_dec = true;
    first_plain = dec.kind != kDecideDone && dec.qmask == 0;
  }
  SeedLabels seed_labels;
  for (int s = 0; s < 64; ++s) seed_labels.p[s] = a.label[s];
  hipLaunchKernelGGL(batch_seed_kernel, dim3(1), dim3(kBlock), 0, st, seen, first_plain ? (u64*)nullptr : words(0), seeds, seed_labels, k);
  GRB_HIP_TRY(hipGetLastError());
  if (first_plain) {
    dec.kind = kDecideHost;
    slots.first_plain();                                    // no seed words: the sources' own labels are direct ones
  }
  GRB_HIP_TRY(hipEventRecord(buf.ev0, st));
  return GRB_SUCCESS;
}

// the level's decision -- the one the totals kernel of the level before published, else the host's; false: no live source
bool Sweep::decide() {
  t_lvl = knobs.trace ? now_us() : 0.0;
  if (!have_dec) dec = batch_decide(nf_s, mf_s, rule, true);
  have_dec = false;
  if (dec.kind == kDecideDone) return false;
  P = dec.pmask; Q = dec.qmask;
  pushed_edges = dec.pushed_edges;
  a.qmask = Q; a.pmask = P;
  a.claims = 0; a.stash = 0;
  a.fcur = words(slots.frontier());
  a.ctl = nullptr;
  a.list_len = nullptr;
  a.big_index = nullptr; a.list = nullptr; a.list_fw = nullptr;
  return true;
}

// ---- every live source pushed and few edges to push: this level and the light ones after it in one launch.  Leaves iter
// at the level the launch ended on and light_status at its status: 0 nothing new (the traversals are over), else capped
// or grown heavy again.
grb_info Sweep::light_launch() {
  pulled_ahead = false;                                     // (launched ahead, the pull kernels found this out and wrote nothing: the plan is dropped)
  int xi[3];
  slots.light_pick(xi);
  // the next clean state block; a fifth launch in one sweep and every later one clear the last block for themselves
  const bool clean_state = tail_states_used < kTailStates;
  TailArgs t;
  tail_carve(t, buf.tail, z, clean_state ? tail_states_used : kTailStates - 1);
  ++tail_states_used;
  t.f0 = a.fcur;
  for (int i = 0; i < 3; ++i) t.X[i] = words(xi[i]);
  t.box = g_box_d;
  t.status = d_ctl + 3;
  t.seq = ++g_box_seq;
  t.iter0 = iter;
  t.max_niter = max_niter;
  t.edge_limit = (unsigned long long)tail_edges;
  t.per_source = per ? 1 : 0;
  a.direct_labels = 1;
  if (!clean_state) GRB_HIP_TRY(hipMemsetAsync(t.st, 0, z.tail_state, st));
  for (int i = 0; i < 3; ++i)
    if (!slots.clean(xi[i])) GRB_HIP_TRY(hipMemsetAsync(t.X[i], 0, sizeof(u64) * (size_t)n, st));
  hipLaunchKernelGGL(batch_tail_kernel, dim3(c.num_cu), dim3(kPThreads), 0, st, a, t);
  GRB_HIP_TRY(hipGetLastError());
  // the label pass behind it, before the host has the box: it reads the launch's status from the control block and
  // leaves at once when the sweep goes on.  A light-level launch adds no kept level, so its arguments are known.
  if (ahead) GRB_TRY(launch_labels(d_ctl + 3));
  GRB_TRY(wait_box());                                       // any number of levels; GRB_PANIC: a grid barrier gave up
  const u64* const h_box = g_box_h;
  const int done = (int)h_box[kBatchCounters + 1];
  light_status = (int)h_box[kBatchCounters + 4];
  labels_done = ahead && light_status != 2;
  edges += h_box[kBatchCounters + 2];
  reached += h_box[kBatchCounters + 3];
  any_left = false;
  for (int s = 0; s < k; ++s) {
    nf_s[s] = h_box[2 + 2 * s];
    mf_s[s] = h_box[3 + 2 * s];
    if (nf_s[s]) any_left = true;
    if (per) {
      reached_s[s] += h_box[kBatchBoxPer + 2 * s];
      edges_s[s] += h_box[kBatchBoxPer + 2 * s + 1];
      const int lp = (int)h_box[kBatchBoxPer + 128 + s];
      if (lp > last_prod[s]) { last_prod[s] = lp; dir_s[s] = 0; }
    }
  }
  levels += done;
  last_dir = 0;
  big_out_new = -1;
  slots.light_done(xi, done, light_status);                 // the last level run, j = done - 1, wrote X[j % 3]: the new frontier
  tail_fresh = false;
  if (knobs.trace) {
    u64 ts[64];
    GRB_HIP_TRY(hipMemcpy(ts, &t.st->ts[0], sizeof(ts), hipMemcpyDeviceToHost));
    fprintf(stderr, "  launch stamps (us from start; prologue, barrier, then per level: work, flush, barrier):");
    for (int i = 1; i < 64 && ts[i]; ++i) fprintf(stderr, " %.1f", (double)(ts[i] - ts[0]) * 0.01);
    fprintf(stderr, "\n");
    fprintf(stderr, "batch levels %d..%d: one launch (light levels), status %d, pairs %llu  %.1f us\n", iter, iter + done - 1,
            light_status, (unsigned long long)h_box[kBatchCounters + 3], now_us() - t_lvl);
  }
  iter += done - 1;
  return GRB_SUCCESS;
}

// ---- a level of the host loop.  Its words' place, then the pull: the first level's plain launch, the kernels already
// launched ahead, the pull kernels for Q, the pull kernel's stash path, or a fill.
grb_info Sweep::pull_stage() {
  const SlotPlan slot = pulled_ahead ? planned : slots.plan();
  slots.commit(slot, iter);                                 // a level of this loop: the plan holds
  a.fnext = words(slot.slot);
  a.new_label = (float)(iter + 1);
  a.direct_labels = slot.keep ? 0 : 1;
  plain_level = first_plain && iter == 1;
  // heavy: as whoever decided the level published it (the totals kernel, or batch_decide here) -- never derived a second
  // time, the pull kernels launched ahead have already stashed by it.  The first level's plain launch claims directly.
  heavy = dec.stash != 0 && !plain_level;
  a.stash = heavy ? dec.stash : 0ull;
  if (plain_level) {
    // the sources' rows, a wave per piece, into slot 0: the fill at the sweep's start has zeroed it
    FirstPieces fp;
    first_level_pieces(A->h_csr_ptr.data(), seeds.v, k, kFirstPiece, fp.pre);
    hipLaunchKernelGGL(batch_first_level_kernel, dim3(fp.pre[k] > 0 ? (fp.pre[k] + kWavesPerBlock - 1) / kWavesPerBlock : 1u), dim3(kBlock),
                       0, st, a, seeds, fp);
    GRB_HIP_TRY(hipGetLastError());
  } else if (pulled_ahead) {
    // the pull kernels are already running, or done: for Q == 0 they have zeroed the words
  } else if (Q) {
    if (H > 0 && !tail_fresh) {
      HotCopy hc = {const_cast<u64*>(a.fcur), A->batch_hot.d_hubs, n, H};
      hipLaunchKernelGGL(batch_hot_refresh_kernel, dim3(hot_copy_blocks(H)), dim3(kBlock), 0, st, hc);
      GRB_HIP_TRY(hipGetLastError());
      if (knobs.trace) fprintf(stderr, "sweep hot block: level %d pulls behind a copy launch of its own\n", iter);
    }
    GRB_TRY(launch_pull(a));
  } else if (heavy) {
    // nothing pulled, but the stash is wanted: the pull kernel's qmask == 0 path writes seen & stash where the fill
    // wrote zeros (it reads no CSC array, so a push-only matrix takes it too)
    hipLaunchKernelGGL(batch_pull_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    GRB_HIP_TRY(hipGetLastError());
  } else {
    GRB_HIP_TRY(hipMemsetAsync(a.fnext, 0, sizeof(u64) * (size_t)n, st));
  }
  pulled_ahead = false;
  return GRB_SUCCESS;
}

// the level's push, for the sources in P: the push kernel, the big rows by their ranges' owners or by slices, the commit
grb_info Sweep::push_stage() {
  if (!P || plain_level) return GRB_SUCCESS;
  const BatchSlices& B = A->batch_out;
  a.big = batch_big(false);
  a.claims = heavy ? 1 : 0;                                 // claims only: the new bits are read back against the stashed old ones
  a.slices = B.d_slices; a.nslices = B.nslices; a.bigrows = B.d_rows; a.nbig = B.nbig;
  const bool big_rows = B.nslices > 0 && big_out_new != 0;  // none in the frontier: no slice or owner kernel has anything to do
  const bool owners = big_rows && heavy && knobs.owner && B.d_range_off && B.d_big_index;
  if (owners) {
    // heavy level: the big rows' edges are settled by the owners of their destination ranges, in LDS; the push kernel
    // lists the big frontier rows it skips
    a.big_index = B.d_big_index; a.list = list.ids; a.list_fw = list.words;
    a.list_len = list.len;                                  // zero here; the commit kernel below puts it back to zero
  }
  hipLaunchKernelGGL(batch_push_kernel, dim3(grid), dim3(kBlock), 0, st, a);
  GRB_HIP_TRY(hipGetLastError());
  a.big_index = nullptr;
  if (owners) {
    // Few narrow ranges (fewer than CUs: a launch of them cannot occupy the chip, whatever its occupancy per CU -- on
    // RMAT-22 it is ONE workgroup, the hub range, walking its pieces of every listed row for 20 us while the wide
    // instance waits): one launch of the wide instance over all ranges, which handles a range of <= 2 Ki rows as it
    // stands.  The ids are taken from their start, narrow ranges first, so the long hub workgroups start first.  The
    // XCD dealing of make_slices holds up to a rotation: the wide part's eighths land on XCDs rotated by nsmall mod 8,
    // each still contiguous on one XCD.  GRB_BATCH_OWNER_MERGE=0: always the two launches (A/B runs, tests).
    const bool merged = knobs.owner_merge && B.nsmall > 0 && B.nranges > B.nsmall && B.nsmall < c.num_cu;
    if (merged) {
      launch_owners<kOwnRows, 1024>(a, B, list, 0, B.nranges, st);
    } else {
      if (B.nsmall > 0) launch_owners<kOwnSmallRows, 512>(a, B, list, 0, B.nsmall, st);
      if (B.nranges > B.nsmall) launch_owners<kOwnRows, 1024>(a, B, list, B.nsmall, B.nranges - B.nsmall, st);
    }
    GRB_HIP_TRY(hipGetLastError());
    if (knobs.trace) {
      unsigned int hc = 0, parts[kListSegs * kListLenStride];
      GRB_HIP_TRY(hipMemcpy(parts, list.len, kListHeader, hipMemcpyDeviceToHost));
      for (int g = 0; g < kListSegs; ++g) hc += parts[g * kListLenStride];
      fprintf(stderr, "batch level %d: owner-computes push, %u of %d big rows in the frontier, %d ranges (%d narrow, %d wide)\n", iter, hc, B.nbig,
              B.nranges, B.nsmall, B.nranges - B.nsmall);
      const int launches = merged ? 1 : (B.nsmall > 0 ? 1 : 0) + (B.nranges > B.nsmall ? 1 : 0);
      fprintf(stderr, "batch level %d: range owners in %d launch%s\n", iter, launches, launches == 1 ? "" : "es");
    }
  } else if (big_rows) {
    hipLaunchKernelGGL(batch_push_slices_kernel, dim3(stream_grid((long long)B.nslices * kWave, kBlock)), dim3(kBlock),
                       0, st, a);
    GRB_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(batch_push_commit_kernel, dim3(grid), dim3(kBlock), 0, st, a);
  GRB_HIP_TRY(hipGetLastError());
  if (knobs.trace)
    fprintf(stderr, "batch push stage of level %d: batch_push_kernel, %sbatch_push_commit_kernel\n", iter,
            owners ? "range owners, " : big_rows ? "batch_push_slices_kernel, " : "");
  return GRB_SUCCESS;
}

// the level's totals and the next level's decision, on the device; behind them the next level's pull, launched ahead
grb_info Sweep::totals_and_ahead() {
  DecideArgs da;
  da.rule = rule;
  da.iteration_left = iter + 1 <= max_niter ? 1 : 0;
  da.open_complete = P == 0 && Q != 0 ? 1 : 0;              // every live source pulled: the level's U covers them all
  da.ctl = d_ctl;
  const HotCopy hc = {a.fnext, A->batch_hot.d_hubs, n, Hcopy};   // the level's words are complete here: their tail, for the next level's pull
  hipLaunchKernelGGL(batch_totals_kernel, dim3(1 + hot_copy_blocks(Hcopy)), dim3(kBlock), 0, st, a.counters, g_box_d, ++g_box_seq, da, hc);
  GRB_HIP_TRY(hipGetLastError());
  tail_fresh = true;
  if (ahead && iter + 1 <= max_niter) {
    // the next level's pull kernels, behind the totals kernel that decides whether and on which bits they run
    BatchArgs an = a;
    an.fcur = a.fnext;
    planned = slots.plan();
    an.fnext = words(planned.slot);
    an.new_label = (float)(iter + 2);
    an.direct_labels = planned.keep ? 0 : 1;
    an.claims = 0; an.stash = 0;
    an.list_len = nullptr;
    an.qmask = 0; an.pmask = 0;
    an.ctl = d_ctl;
    GRB_TRY(launch_pull(an));
    pulled_ahead = true;
  }
  return GRB_SUCCESS;
}

// the host blocks here: the level's counters and the next level's decision out of the box
grb_info Sweep::read_level() {
  GRB_TRY(wait_box());
  const u64* const h_box = g_box_h;
  u64 t[kBatchCounters];
  for (int j = 0; j < kBatchCounters; ++j) t[j] = __atomic_load_n(&h_box[j], __ATOMIC_RELAXED);
  dec.qmask = __atomic_load_n(&h_box[kBoxDecision], __ATOMIC_RELAXED);
  dec.pmask = __atomic_load_n(&h_box[kBoxDecision + 1], __ATOMIC_RELAXED);
  dec.kind = (int)__atomic_load_n(&h_box[kBoxDecision + 2], __ATOMIC_RELAXED);
  dec.stash = __atomic_load_n(&h_box[kBoxDecision + 3], __ATOMIC_RELAXED);
  have_dec = true;
  if ((t[kCntInOpen] & kInOpenCounted) && (t[kCntInOpen] & (kInOpenCounted - 1)) == 0) in_done = true;
  big_out_new = (long long)t[kCntBigOut];
  ++levels;
  last_dir = Q ? 1 : 0;
  any_left = false;
  u64 pairs = 0;
  for (int s = 0; s < k; ++s) {
    nf_s[s] = t[2 + 2 * s];
    mf_s[s] = t[3 + 2 * s];
    pairs += nf_s[s];
    reached += nf_s[s];
    edges += mf_s[s];
    reached_s[s] += nf_s[s];
    edges_s[s] += mf_s[s];
    if (nf_s[s]) { any_left = true; last_prod[s] = iter; dir_s[s] = (int)((Q >> s) & 1ull); }
  }
  if (knobs.trace)
    fprintf(stderr, "batch level %d: pull %d sources, push %d (%.0f edges, %s) -> vertices %llu pairs %llu, big in-rows open %s%llu, "
            "big out-rows found %lld, next level %s  %.1f us, U %llu%s\n",
            iter, __builtin_popcountll(Q), __builtin_popcountll(P), pushed_edges, a.claims ? "claims" : "direct", t[0],
            pairs, (t[kCntInOpen] & kInOpenCounted) ? "" : "(not counted) ", t[kCntInOpen] & (kInOpenCounted - 1), big_out_new,
            dec.kind == kDecideHost ? (pulled_ahead ? "pulled ahead" : "host") : dec.kind == kDecideLight ? "light" : "none",
            now_us() - t_lvl, t[kCntOpenU] & (kOpenUComplete - 1), (t[kCntOpenU] & kOpenUComplete) ? "" : " (not complete)");
  dec.pushed_edges = 0;
  for (int s = 0; s < k; ++s) if ((dec.pmask >> s) & 1ull) dec.pushed_edges += (double)mf_s[s];
  return GRB_SUCCESS;
}

// the depth vectors, the sweep's time, what the next sweep may rely on, the results
grb_info Sweep::finish(int* per_dir, SweepTotals* out) {
  const bool hit_cap = iter > max_niter && any_left;
  // (unless the pass enqueued behind the closing light-level launch has written them)
  if (!labels_done) GRB_TRY(launch_labels(nullptr));
  if (hit_cap && slots.any_direct()) {
    // vertices discovered by the last allowed iteration are never assigned by the reference loop (bfs.hpp:48-66)
    hipLaunchKernelGGL(batch_unlabel_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, a,
                       (float)(max_niter + 1));
    GRB_HIP_TRY(hipGetLastError());
  }
  float ms = 0.f;
  GRB_HIP_TRY(hipEventRecord(buf.ev1, st));
  GRB_HIP_TRY(hipEventSynchronize(buf.ev1));                // the labels are in place
  GRB_HIP_TRY(hipEventElapsedTime(&ms, buf.ev0, buf.ev1));
  buf.zero->keep(n, z.stride, z.nstore, slots.clean_flags());
  if (own) {
    own->small_clean = true;
  } else {
    g_sweep_scratch.epoch = c.slot_epoch[7];
    g_sweep_scratch.ptr = buf.words;
  }
  if (per)
    for (int s = 0; s < k; ++s) {
      const int lv = last_prod[s] + 1;
      per[s].levels = lv < max_niter ? lv : max_niter;
      per[s].tight_ms = ms / (float)k;
      per[s].edges_traversed = (int64_t)edges_s[s];
      per[s].reached = (int32_t)(reached_s[s] > 0x7fffffffull ? 0x7fffffff : reached_s[s]);
      if (per_dir) per_dir[s] = dir_s[s];
    }
  out->levels = levels; out->last_dir = last_dir; out->edges = edges; out->reached = reached; out->hit_cap = hit_cap; out->ms = ms;
  return GRB_SUCCESS;
}

// k traversals of A (both orientations, the pull hint and the slice tables ready) from sources[] into v[] under the rules
// (mode, max_niter, switchpoint).  per != nullptr: every source's own result block, as its own one-launch traversal
// would report it -- reached = 1 + its discoveries, edges = its out-degree + theirs, levels = the iterations its own loop
// runs (up to and including the first that discovers nothing, at most max_niter), tight_ms = the sweep's device time / k;
// per_dir[s] = 1 when the source's last productive level was pulled.  Timed with HIP events of its own (the library's
// timer belongs to the caller); returns after the label pass has completed.
static grb_info batch_sweep(grb_vector* v, int k, grb_matrix A, const grb_index* sources, int rules_mode, int max_niter,
                            float switchpoint, SweepOwn* own, grb_bfs_result* per, int* per_dir, SweepTotals* out) {
  Sweep s(k, A, max_niter, own, per);
  GRB_TRY(s.begin(v, sources, rules_mode, switchpoint));
  for (; s.iter <= max_niter; ++s.iter) {
    if (!s.decide()) break;                                 // no live source
    if (s.dec.kind == kDecideLight) {
      GRB_TRY(s.light_launch());
      if (s.light_status == 0) break;                       // nothing new: the traversals are over
      continue;                                             // capped (the loop condition ends it) or grown heavy again
    }
    GRB_TRY(s.pull_stage());
    GRB_TRY(s.push_stage());
    GRB_TRY(s.totals_and_ahead());
    GRB_TRY(s.read_level());
    if (!s.any_left) break;
  }
  return s.finish(per_dir, out);
}

// ---- the sweep as the traversal queue uses it (bfs_persist.hip: bfs_co_flush) ------------------------------------------
// Every batch_* kernel launched once on nothing (n = 0, no slices, an empty list), so that no sweep pays a kernel's first
// launch: the code object is loaded by the first, the others are looked up.  The owner-computes kernels run over the
// matrix's real ranges with an empty list of big rows (they clear their LDS and find nothing to write back).
static grb_info sweep_warm(grb_matrix A, SweepOwn* own, const SweepSizes& z) {
  Context& c = ctx();
  hipStream_t st = c.stream;
  GRB_TRY(batch_box());
  BatchArgs a;
  memset(&a, 0, sizeof(a));
  a.optr = A->csr.ptr; a.oind = A->csr.ind; a.iptr = A->csc.ptr; a.iind = A->csc.ind;
  a.hint = A->d_pull_hint;
  a.n = 0;
  a.seen = (u64*)own->words; a.fcur = (const u64*)own->words; a.fnext = (u64*)own->words;
  a.big = batch_big(true);
  a.big_out = batch_big(false);
  a.counters = (u64*)own->cnt;
  a.direct_labels = 1;
  const ListBlock list = list_carve(own->list, z);
  GRB_HIP_TRY(hipMemsetAsync(own->cnt, 0, sizeof(u64) * kBatchSlots * kBatchCounters, st));
  GRB_HIP_TRY(hipMemsetAsync(list.len, 0, kListHeader, st));   // the list's lengths: 0
  if (!own->warmed) {
    SeedSources none;
    memset(&none, 0, sizeof(none));
    SeedLabels no_labels;
    memset(&no_labels, 0, sizeof(no_labels));
    FirstPieces no_pieces;
    memset(&no_pieces, 0, sizeof(no_pieces));
    hipLaunchKernelGGL(batch_seed_kernel, dim3(1), dim3(kBlock), 0, st, a.seen, a.seen, none, no_labels, 0);
    hipLaunchKernelGGL(batch_first_level_kernel, dim3(1), dim3(kBlock), 0, st, a, none, no_pieces);   // k = 0: no piece
    hipLaunchKernelGGL(batch_pull_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_pull_slices_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_big_apply_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_push_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_push_slices_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_push_commit_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_unlabel_kernel, dim3(1), dim3(kBlock), 0, st, a, 0.f);
    LabelArgs L;
    memset(&L, 0, sizeof(L));
    L.seen = a.seen;
    hipLaunchKernelGGL(batch_labels_kernel, dim3(1), dim3(kBlock), 0, st, L);
    GRB_HIP_TRY(hipGetLastError());
    // the light-level launch on an empty queue: one level that finds nothing, the grid barrier at its real width
    TailArgs t;
    memset(&t, 0, sizeof(t));
    t.f0 = a.fcur;
    for (int i = 0; i < 3; ++i) t.X[i] = a.seen;
    tail_carve(t, own->tail, z, 0);
    t.box = g_box_d;
    t.status = a.counters + kBatchSlots * kBatchCounters + 3;
    t.seq = ++g_box_seq;
    t.iter0 = 1; t.max_niter = 1;
    t.per_source = 1;
    GRB_HIP_TRY(hipMemsetAsync(t.st, 0, z.tail_state, st));
    hipLaunchKernelGGL(batch_tail_kernel, dim3(c.num_cu), dim3(kPThreads), 0, st, a, t);
    GRB_HIP_TRY(hipGetLastError());
    DecideArgs da;
    memset(&da, 0, sizeof(da));                             // no source: the decision is "done"
    da.ctl = a.counters + kBatchSlots * kBatchCounters;
    HotCopy no_hubs;
    memset(&no_hubs, 0, sizeof(no_hubs));
    hipLaunchKernelGGL(batch_totals_kernel, dim3(1), dim3(kBlock), 0, st, a.counters, g_box_d, ++g_box_seq, da, no_hubs);
    hipLaunchKernelGGL(batch_hot_refresh_kernel, dim3(1), dim3(kBlock), 0, st, no_hubs);
    GRB_HIP_TRY(hipGetLastError());
    a.ctl = da.ctl;                                         // ... and the pull kernels as a launch ahead of it finds them: they leave at once
    hipLaunchKernelGGL(batch_pull_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_pull_slices_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(batch_big_apply_kernel, dim3(1), dim3(kBlock), 0, st, a);
    GRB_HIP_TRY(hipGetLastError());
    a.ctl = nullptr;
  }
  // one workgroup of each owner-computes instance, once per process, on the first matrix that has such ranges
  const BatchSlices& B = A->batch_out;
  if (B.d_range_off && B.nranges > 0) {
    a.nbig = B.nbig;
    if (B.nsmall > 0 && !own->warmed_own_small) {
      launch_owners<kOwnSmallRows, 512>(a, B, list, 0, 1, st);
      own->warmed_own_small = true;
    }
    if (B.nranges > B.nsmall && !own->warmed_own_wide) {
      launch_owners<kOwnRows, 1024>(a, B, list, B.nsmall, 1, st);
      own->warmed_own_wide = true;
    }
    GRB_HIP_TRY(hipGetLastError());
  }
  GRB_HIP_TRY(hipStreamSynchronize(st));
  if (__atomic_load_n(&g_box_h[kBatchCounters], __ATOMIC_ACQUIRE) != g_box_seq) return GRB_PANIC;
  own->warmed = true;
  own->small_clean = true;                                  // the totals kernel left the counters zero; the list's length was set to zero above
  return GRB_SUCCESS;
}

static grb_info sweep_grow(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return GRB_SUCCESS;
  if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
  const size_t want = (bytes + bytes / 8 + 255) & ~(size_t)255;
  GRB_HIP_TRY(hipMalloc(p, want));
  *cap = want;
  return GRB_SUCCESS;
}

// Once per matrix, at its first gathered launch under the width rule: the slice and owner-range tables of both orientations, the
// sweep's own buffers (kept from matrix to matrix, grown for a larger one; new memory within a quarter of what the device
// has free) and the first launch of its kernels.  A->sweep_state: 1 the queue may sweep this matrix, -1 it may not.
// The attempt is made once: whatever stops it -- the memory rule at that moment included -- leaves the route off for this
// matrix until it is built again (a retry at every launch would put an allocation attempt in front of every traversal).
grb_info grb::bfs_sweep_provision(grb_matrix A) {
  if (A->sweep_state != 0) return A->sweep_state > 0 ? GRB_SUCCESS : GRB_NOT_IMPLEMENTED;
  A->sweep_state = -1;
  if (A->format != 0 || A->csc_alias || !A->csr.ptr || !A->csc.ptr || A->nrows != A->ncols || A->nrows < 1) return GRB_NOT_IMPLEMENTED;
  if ((Index)A->h_csr_ptr.size() != A->nrows + 1 || (Index)A->h_csc_ptr.size() != A->nrows + 1) return GRB_NOT_IMPLEMENTED;
  auto failed = [](grb_info i) { (void)hipGetLastError(); return i; };
  Context& c = ctx();
  SweepOwn& o = g_sweep;
  // the memory rule first, over everything this call may allocate: the tables of an orientation that has none yet by
  // their upper bounds (at most nvals / big rows, a slice per kBatchPushSlice entries and per row, the owner offsets
  // capped at 128 Mi entries as ensure_slices caps them), then the buffers by their sizes
  size_t grow = 0, list_bound = sweep_sizes(A).list;
  for (int in = 0; in < 2; ++in) {
    if ((in ? A->batch_in : A->batch_out).ready) continue;
    const size_t max_rows = (size_t)(A->nvals / batch_big(in != 0)) + 1;
    const size_t max_slices = (size_t)(A->nvals / (in ? kBatchSlice : kBatchPushSlice)) + max_rows;
    grow += sizeof(int4) * max_slices + sizeof(Index) * max_rows;
    if (!in) {
      list_bound = kListHeader + ((sizeof(int) * kListSegs * max_rows + 255) & ~(size_t)255) + sizeof(u64) * kListSegs * max_rows;   // (the big-row list: SweepSizes::list)
      const size_t max_ranges = (size_t)(3 * 256 + A->nrows / kOwnSmallRows + 2);
      grow += sizeof(Index) * std::min<size_t>(max_rows * (size_t)own_off_stride((long long)max_ranges), (size_t)128 << 20) + 2 * sizeof(Index) * (max_ranges + 1);
      grow += sizeof(int) * (size_t)A->nrows;                // the table vertex -> big index
    }
  }
  // the hot block, when this matrix has none yet: its arrays and the words' tails by the cap on the hubs.  When the rule
  // says no to the sum but yes without them, the matrix is provisioned without a hot block.
  const bool hot_open = !A->batch_hot.ready && batch_hot_cap() > 0;
  bool hot_allowed = true;
  {
    if (o.tail_cap < sweep_sizes(A).tail) grow += sweep_sizes(A).tail + sweep_sizes(A).tail / 8;
    if (o.list_cap < list_bound) grow += list_bound + list_bound / 8;
    const long long Hb = hot_open ? std::min<long long>(batch_hot_cap(), A->nrows) : (long long)A->batch_hot.H;
    auto words_grow = [&](long long H) {
      const size_t w = sweep_sizes(A, H).words;
      return o.words_cap < w ? w + w / 8 : (size_t)0;
    };
    const size_t with_hot = grow + words_grow(Hb) + (hot_open ? hot_bound(A, Hb) : 0), without = grow + words_grow(hot_open ? 0 : Hb);
    if (with_hot > 0) {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return failed(GRB_OUT_OF_MEMORY);
      if (with_hot + 4096 > free_b / 4) {
        if (!hot_open || (without > 0 && without + 4096 > free_b / 4)) return GRB_OUT_OF_MEMORY;
        hot_allowed = false;
      }
    }
  }
  grb_info i = ensure_pull_hint(&A->d_pull_hint, A->csc, A->csr.ptr, c.stream);
  if (i == GRB_SUCCESS) i = ensure_slices(A, true);
  if (i == GRB_SUCCESS) i = ensure_slices(A, false);
  if (i != GRB_SUCCESS) return failed(i);
  ensure_hot(A, hot_allowed);
  SweepSizes z = sweep_sizes(A);
  if (o.words_cap < z.words || o.tail_cap < z.tail || o.list_cap < z.list) {
    if (hipStreamSynchronize(c.stream) != hipSuccess) return failed(GRB_PANIC);   // (an earlier sweep may still read the old ones)
    o.zero.valid = false;
    o.small_clean = false;
    i = sweep_grow(&o.words, &o.words_cap, z.words);
    if (i != GRB_SUCCESS && A->batch_hot.H > 0) {            // no room for the tails: without the hot block, then
      (void)hipGetLastError();
      hot_drop(A);
      z = sweep_sizes(A);
      i = sweep_grow(&o.words, &o.words_cap, z.words);
    }
    if (i == GRB_SUCCESS) i = sweep_grow(&o.tail, &o.tail_cap, z.tail);
    if (i == GRB_SUCCESS) i = sweep_grow(&o.list, &o.list_cap, z.list);
    if (i != GRB_SUCCESS) return failed(i);
  }
  if (!o.cnt) {
    if (hipMalloc(&o.cnt, sizeof(u64) * (kBatchSlots * kBatchCounters + kBatchCtlWords)) != hipSuccess) return failed(GRB_OUT_OF_MEMORY);
  }
  if (!o.ev0) {
    if (hipEventCreate(&o.ev0) != hipSuccess || hipEventCreate(&o.ev1) != hipSuccess) return failed(GRB_PANIC);
  }
  i = sweep_warm(A, &o, z);
  if (i != GRB_SUCCESS) return failed(i);
  A->sweep_state = 1;
  return GRB_SUCCESS;
}

// k (2 .. 64) queued traversals of a provisioned matrix as one sweep on the sweep's own buffers; per[s] and per_dir[s] as
// batch_sweep leaves them.  Anything but GRB_SUCCESS: the vectors hold nothing to rely on, the caller runs the traversals
// some other way.
grb_info grb::bfs_sweep_routed(grb_vector* v, int k, grb_matrix A, const grb_index* sources, int mode, int max_niter, float switchpoint,
                               grb_bfs_result* per, int* per_dir) {
  if (k < 1 || k > 64 || A->sweep_state != 1) return GRB_NOT_IMPLEMENTED;
  SweepTotals tot;
  GRB_TRY(batch_sweep(v, k, A, sources, mode, max_niter, switchpoint, &g_sweep, per, per_dir, &tot));
  return tot.hit_cap ? GRB_NOT_IMPLEMENTED : GRB_SUCCESS;
}

extern "C" grb_info grb_bfs_batch(grb_vector* v, int k, grb_matrix A, const grb_index* sources, grb_descriptor desc,
                                  grb_bfs_result* result) { GRB_API_ENTER();
  if (!v || !A || !desc || !sources) return GRB_UNINITIALIZED_OBJECT;
  if (k < 1 || k > 64) return GRB_INVALID_VALUE;
  if (!A->built || !A->csr.ptr || !A->csc.ptr) return GRB_UNINITIALIZED_OBJECT;
  if (A->nrows != A->ncols) return GRB_DIMENSION_MISMATCH;
  const Index n = A->nrows;
  for (int s = 0; s < k; ++s) {
    if (!v[s]) return GRB_UNINITIALIZED_OBJECT;
    if (v[s]->dtype != GRB_F32) return GRB_DOMAIN_MISMATCH;
    if (v[s]->nsize != n) return GRB_DIMENSION_MISMATCH;
    if (sources[s] < 0 || sources[s] >= n) return GRB_INVALID_INDEX;
  }
  GRB_TRY(ctx_init());
  hipStream_t st = ctx().stream;
  GRB_TRY(ensure_pull_hint(&A->d_pull_hint, A->csc, A->csr.ptr, st));
  GRB_TRY(ensure_slices(A, true));
  GRB_TRY(ensure_slices(A, false));
  ensure_hot(A);
  SweepTotals tot;
  GRB_TRY(batch_sweep(v, k, A, sources, desc->desc[GRB_MXVMODE], desc->max_niter, desc->switchpoint, nullptr, nullptr, nullptr, &tot));
  desc->lastmxv = tot.last_dir ? GRB_PULLONLY : GRB_PUSHONLY;
  if (result) {
    result->levels = tot.levels;
    result->tight_ms = tot.ms;
    result->edges_traversed = tot.hit_cap ? -1 : (int64_t)tot.edges;   // under a cap the tally would count unassigned vertices
    result->reached = tot.hit_cap ? -1 : (int32_t)(tot.reached > 0x7fffffffull ? 0x7fffffff : tot.reached);
  }
  return GRB_SUCCESS;
}
