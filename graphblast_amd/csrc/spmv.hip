// spmv.hip -- the pull half of mxv/vxm on gfx950.
//
//  k_spmv            generic semiring SpMV  w[i] = (+)_j A[i,j] (x) u[j]  with the optional
//                    mask / accum epilogue of backend/cuda/spmv.hpp:178-220.  The reference
//                    delegates to moderngpu's merge-path SpmvCsrBinary (source not in the
//                    mount); this is a different design, built for what bounds the kernel on
//                    MI355X -- not the 8 B/nonzero matrix stream but the 4 B gathers of u:
//                      * rows are cut at build time into wave tiles of <= 512 nonzeros and
//                        <= 64 rows; rows longer than a tile become slices that each produce
//                        one partial, folded in slice order by a second tiny kernel
//                        (deterministic, no atomics);
//                      * the columns are ranked by reference count once per matrix and u is
//                        packed by that rank on every launch, so the hot values form a dense
//                        prefix: 32 Ki of them live in LDS, the warm tail stays L2-resident;
//                      * one persistent 1024-thread workgroup per CU, 16 independent waves,
//                        each with three tiles in flight (stream / gather / reduce).
//  k_spmv_masked_or  Boolean pull step with fused mask (kernels/spmv.hpp:10-59, all eight
//                    <Scmp, EarlyExit, OpReuse> variants): one 64-lane wave owns 64
//                    consecutive rows, lanes first probe their own row serially (the common
//                    early-exit case) and rows still undecided after kSerialProbe neighbours
//                    are finished cooperatively by the whole wave with coalesced index reads
//                    and a ballot, which bounds the divergence a hub row can cause.
//
// Algorithmic bytes per launch of k_spmv: 8*nnz + 12*n + 4.
#include "common.hpp"
#include <chrono>

namespace grb {

// tuning knobs of the SpMV kernel (tools/build_spmv_variants.sh builds A/B variants)
#ifndef GRB_HUB_THREADS
#define GRB_HUB_THREADS 1024
#endif
#ifndef GRB_HUB_HOT
#define GRB_HUB_HOT 32768
#endif
#ifndef GRB_HUB_NT
#define GRB_HUB_NT 1
#endif
constexpr int kHubThreads = GRB_HUB_THREADS;   // one workgroup per CU owning all 160 KiB of LDS
constexpr int kHubWaves = kHubThreads / kWave;
// kWaveTile (GRB_HUB_TILE), the nonzeros per wave tile, lives in common.hpp: spmm.hip walks the same tiles
constexpr int kWaveRows = 64;       // rows per wave tile: lane r carries the pointers of row r
constexpr int kHot = GRB_HUB_HOT;   // leading values of the packed vector kept in LDS (128 KiB)
constexpr int kHubPerCu = 163840 / (4 * kHot + 4 * kHubWaves * kWaveTile);
static_assert(kHubPerCu >= 1, "SpMV kernel LDS budget");
template <typename V>
__device__ inline V stream_load(const V* p) {
#if GRB_HUB_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

template <int SR, typename T>
__device__ inline void spmv_store(T* w, Index row, T value, const void* mask, int mask_f32, int scmp, int accum);

}  // namespace grb
#include "spmv_bands.hpp"
#include "spmv_cband.hpp"
#include <algorithm>
namespace grb {

// ---- plan ---------------------------------------------------------------------------
template <typename V>
static grb_info to_device(const std::vector<V>& h, V** d) {
  if (h.empty()) return GRB_SUCCESS;
  GRB_HIP_TRY(hipMalloc(d, sizeof(V) * h.size()));
  GRB_HIP_TRY(hipMemcpy(*d, h.data(), sizeof(V) * h.size(), hipMemcpyHostToDevice));
  return GRB_SUCCESS;
}

grb_info build_spmv_plan(const std::vector<Index>& ptr, Index n, Index nminor, SpmvPlan* plan) {
  free_spmv_plan(plan);
  plan->nminor = nminor;
  plan->nrows = n;
  std::vector<SpmvBlock> tiles;
  std::vector<int> long_row, long_slot_ptr;
  int nslots = 0;
  Index r = 0;
  while (r < n) {
    const Index len = ptr[r + 1] - ptr[r];
    if (len > kWaveTile) {
      long_row.push_back(r);
      long_slot_ptr.push_back(nslots);
      for (Index s = ptr[r]; s < ptr[r + 1]; s += kWaveTile) {
        const Index e = s + kWaveTile < ptr[r + 1] ? s + kWaveTile : ptr[r + 1];
        tiles.push_back(SpmvBlock{r, r + 1, s, e, nslots++});
      }
      ++r;
      continue;
    }
    const Index start = r;
    Index nnz = 0;
    while (r < n && r - start < kWaveRows) {
      const Index l = ptr[r + 1] - ptr[r];
      if (nnz + l > kWaveTile) break;
      nnz += l;
      ++r;
    }
    tiles.push_back(SpmvBlock{start, r, ptr[start], ptr[r], -1});
  }
  long_slot_ptr.push_back(nslots);
  plan->ntiles = (int)tiles.size();
  plan->nlong = (int)long_row.size();
  plan->nslots = nslots;
  GRB_TRY(to_device(tiles, &plan->d_tiles));
  if (plan->nlong) {
    GRB_TRY(to_device(long_row, &plan->d_long_row));
    GRB_TRY(to_device(long_slot_ptr, &plan->d_long_slot_ptr));
    GRB_HIP_TRY(hipMalloc(&plan->d_partials, 4 * (size_t)nslots));
  }
  return GRB_SUCCESS;
}

void free_spmv_plan(SpmvPlan* plan) {
  void* ptrs[] = {plan->d_tiles, plan->d_long_row, plan->d_long_slot_ptr, plan->d_partials,
                  plan->d_ind2, plan->d_order, plan->d_u2};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  free_spmv_bands(plan->bands);
  free_spmv_cband(plan->cband);
  *plan = SpmvPlan();
}

// The stored values were rewritten in place (grb_matrix_set_values, matrix (x) scalar / vector): the two band
// formats keep private copies of the values (or one iso value) taken at their first product, so they go; the
// next product prepares them again from the live arrays.  The tiles and the renamed column ids hold structure only.
void spmv_plan_values_changed(SpmvPlan* plan) {
  free_spmv_bands(plan->bands);
  free_spmv_cband(plan->cband);
  plan->bands = nullptr;
  plan->cband = nullptr;
  plan->cband_tried = false;
}

// ---- hub packing ----------------------------------------------------------------------
// Power-law graphs send most gathers to a small set of columns (RMAT-22: the 32 Ki most
// referenced columns take 52 % of the nonzeros, the top 1 Mi take 97 %), but their entries of
// u are scattered over the whole vector, so every hot value drags a mostly-cold 128 B line
// through L2 and the gather stream runs at the fabric rate (measured: 9.3 GB of HBM traffic per
// launch against 1.08 GB algorithmic).  The first SpMV of an orientation therefore ranks the
// columns by reference count and keeps a private copy of the column ids renamed by rank.
// Each launch packs u by that order (one 4 B gather per column), which puts the hot values
// in a dense prefix: the first kHot of them are staged in LDS by every workgroup and the next
// few hundred thousand stay L2-resident.  The row sums are formed in the same order as
// before, so results are bit-identical to the unpacked kernel.
__global__ void rename_columns_kernel(const Index* __restrict__ ind, Index nvals, const Index* __restrict__ rank,
                                      Index* __restrict__ ind2) {
  const Index stride = (Index)gridDim.x * blockDim.x;
  for (Index p = (Index)blockIdx.x * blockDim.x + threadIdx.x; p < nvals; p += stride) ind2[p] = rank[ind[p]];
}

template <typename T>
__global__ void pack_vector_kernel(const T* __restrict__ u, const Index* __restrict__ order, Index n,
                                   T* __restrict__ u2) {
  const Index i = (Index)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) u2[i] = u[order[i]];
}

// Splits the matrix by column rank into `k` bands (spmv_bands.hpp) and builds the tiles of every phase.
// Heavy per-entry work on the device; the tile lists from the piece pointers on the host, like build_spmv_plan.
// LDS prefixes a plan prepared from now on may use: 1 (default) = the one-prefix kernel; GRB_SPMV_BANDS or
// grb_spmv_set_bands raise it.  Off by default: measured -7 % on RMAT-22 at 4 bands against a second copy of the
// matrix, ~0.1 s of preparation and a different (fixed) summation order.
static int g_spmv_bands = -1;
int spmv_bands_setting(int set) {
  if (g_spmv_bands < 0) g_spmv_bands = getenv("GRB_SPMV_BANDS") ? atoi(getenv("GRB_SPMV_BANDS")) : 1;
  if (set > 0) g_spmv_bands = set > kMaxBands ? kMaxBands : set;
  return g_spmv_bands;
}

static int spmv_band_count(Index npacked) {
  const int want = spmv_bands_setting(0);
  int k = (int)((npacked + kHot - 1) / kHot);
  if (k > want) k = want;
  if (k > kMaxBands) k = kMaxBands;
  return k;
}

static grb_info prepare_bands(const CsrArrays& M, SpmvPlan& plan, const Index* d_rank) {
  const Index n = plan.nrows;
  const int k = spmv_band_count(plan.npacked);
  const int G = ctx().num_cu * kHubPerCu;
  if (k < 2 || n < 2 * G || (long long)M.nvals < 64ll * kWaveTile * G) return GRB_SUCCESS;   // too small to cut per workgroup
  hipStream_t st = ctx().stream;
  SpmvBands* B = new SpmvBands();
  struct Guard { SpmvBands* b; ~Guard() { free_spmv_bands(b); } } guard{B};
  std::vector<void*> temp;
  struct TempGuard { std::vector<void*>& v; ~TempGuard() { for (void* p : v) if (p) (void)hipFree(p); } } tguard{temp};
  auto dalloc = [&](size_t bytes, bool keep) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    (keep ? B->owned : temp).push_back(p);
    return p;
  };
  const size_t nb = (size_t)(k - 1) * (size_t)n;             // (band, row) cells of the bands >= 1
  unsigned int* cnt0 = (unsigned int*)dalloc(4 * ((size_t)n + 1), true);     // becomes the main part's row pointers
  unsigned int* cntb = (unsigned int*)dalloc(4 * (nb + 1), false);          // becomes the band stream offsets
  unsigned int* pid = (unsigned int*)dalloc(4 * (nb + 1), false);
  unsigned int* flag = (unsigned int*)dalloc(4 * (nb + 1), false);
  if (!cnt0 || !cntb || !pid || !flag) return GRB_OUT_OF_MEMORY;
  GRB_HIP_TRY(hipMemsetAsync(cnt0 + n, 0, 4, st));
  GRB_HIP_TRY(hipMemsetAsync(cntb + nb, 0, 4, st));
  const int rgrid = stream_grid((long long)n * kWave, kBlock);
  hipLaunchKernelGGL(band_count_kernel, dim3(rgrid), dim3(kBlock), 0, st, M.ptr, M.ind, d_rank, n, k, cnt0, cntb);
  GRB_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(band_flags_kernel, dim3(stream_grid((long long)nb + 1, kBlock)), dim3(kBlock), 0, st,
                     (const unsigned int*)cntb, (long long)nb + 1, flag);
  GRB_HIP_TRY(hipMemcpyAsync(pid, flag, 4 * (nb + 1), hipMemcpyDeviceToDevice, st));
  GRB_TRY(device_exclusive_scan_u32(cnt0, (long long)n + 1));
  GRB_TRY(device_exclusive_scan_u32(cntb, (long long)nb + 1));
  GRB_TRY(device_exclusive_scan_u32(pid, (long long)nb + 1));
  unsigned int nnz0 = 0, nnzb = 0, npieces = 0;
  GRB_HIP_TRY(hipMemcpy(&nnz0, cnt0 + n, 4, hipMemcpyDeviceToHost));
  GRB_HIP_TRY(hipMemcpy(&nnzb, cntb + nb, 4, hipMemcpyDeviceToHost));
  GRB_HIP_TRY(hipMemcpy(&npieces, pid + nb, 4, hipMemcpyDeviceToHost));
  if ((long long)nnz0 + nnzb != (long long)M.nvals) return GRB_PANIC;
  if ((long long)nnzb * 16 < (long long)M.nvals) return GRB_SUCCESS;         // the later prefixes carry < 6 %: not worth a copy
  Index* m0_ind = (Index*)dalloc(4 * (size_t)nnz0, true);
  unsigned int* m0_val = (unsigned int*)dalloc(4 * (size_t)nnz0, true);
  Index* bs_ind = (Index*)dalloc(4 * (size_t)nnzb, true);
  unsigned int* bs_val = (unsigned int*)dalloc(4 * (size_t)nnzb, true);
  Index* piece_ptr = (Index*)dalloc(4 * ((size_t)npieces + 1), true);
  Index* piece_row = (Index*)dalloc(4 * ((size_t)npieces + 1), true);
  if (!m0_ind || !m0_val || !bs_ind || !bs_val || !piece_ptr || !piece_row) return GRB_OUT_OF_MEMORY;
  hipLaunchKernelGGL(band_scatter_kernel, dim3(rgrid), dim3(kBlock), 0, st, M.ptr, M.ind, (const unsigned int*)M.val, d_rank,
                     n, k, (const unsigned int*)cnt0, (const unsigned int*)cntb, (const unsigned int*)pid,
                     (const unsigned int*)flag, m0_ind, m0_val, bs_ind, bs_val, piece_ptr, piece_row);
  GRB_HIP_TRY(hipGetLastError());
  const Index sentinel = (Index)nnzb;
  GRB_HIP_TRY(hipMemcpyAsync(piece_ptr + npieces, &sentinel, 4, hipMemcpyHostToDevice, st));
  GRB_HIP_TRY(hipStreamSynchronize(st));

  // ---- host: the tile lists
  std::vector<Index> ptr((size_t)n + 1), m0((size_t)n + 1), pptr((size_t)npieces + 1), prow((size_t)npieces + 1);
  std::vector<unsigned int> band_first((size_t)k);           // first piece of band b (b >= 1), [k-1] = npieces
  GRB_HIP_TRY(hipMemcpy(ptr.data(), M.ptr, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost));
  GRB_HIP_TRY(hipMemcpy(m0.data(), cnt0, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost));
  GRB_HIP_TRY(hipMemcpy(pptr.data(), piece_ptr, 4 * ((size_t)npieces + 1), hipMemcpyDeviceToHost));
  if (npieces) GRB_HIP_TRY(hipMemcpy(prow.data(), piece_row, 4 * (size_t)npieces, hipMemcpyDeviceToHost));
  for (int b = 1; b < k; ++b)
    GRB_HIP_TRY(hipMemcpy(&band_first[b - 1], pid + (size_t)(b - 1) * n, 4, hipMemcpyDeviceToHost));
  band_first[k - 1] = npieces;

  // rows of more than a tile are sliced in every phase; the others are cut into one range per workgroup,
  // balanced by their nonzeros
  auto is_long = [&](Index r) { return ptr[(size_t)r + 1] - ptr[r] > kWaveTile; };
  long long short_nnz = 0;
  for (Index r = 0; r < n; ++r) if (!is_long(r)) short_nnz += ptr[(size_t)r + 1] - ptr[r];
  std::vector<Index> cut((size_t)G + 1, n);
  {
    long long acc = 0;
    int g = 0;
    cut[0] = 0;
    for (Index r = 0; r < n && g + 1 < G; ++r) {
      if (!is_long(r)) acc += ptr[(size_t)r + 1] - ptr[r];
      while (g + 1 < G && acc * G >= short_nnz * (long long)(g + 1)) cut[++g] = r + 1;
    }
  }
  // slots of the long rows: main slices first, then band 1, ...
  std::vector<int> long_id((size_t)n, -1), long_row, slices_of;
  for (Index r = 0; r < n; ++r)
    if (is_long(r)) { long_id[r] = (int)long_row.size(); long_row.push_back(r); slices_of.push_back(0); }
  auto nslices = [](Index len) { return (int)((len + kWaveTile - 1) / kWaveTile); };
  for (size_t i = 0; i < long_row.size(); ++i) slices_of[i] = nslices(m0[(size_t)long_row[i] + 1] - m0[long_row[i]]);
  for (unsigned int p = 0; p < npieces; ++p)
    if (long_id[prow[p]] >= 0) slices_of[long_id[prow[p]]] += nslices(pptr[(size_t)p + 1] - pptr[p]);
  std::vector<int> slot_ptr(long_row.size() + 1, 0), next_slot(long_row.size());
  for (size_t i = 0; i < long_row.size(); ++i) slot_ptr[i + 1] = slot_ptr[i] + slices_of[i];
  for (size_t i = 0; i < long_row.size(); ++i) next_slot[i] = slot_ptr[i];

  std::vector<SpmvBlock> short_t[kMaxBands], long_t[kMaxBands];
  std::vector<int> short_lo[kMaxBands];
  // main part: every row appears (an empty main part still has to emit t[row])
  {
    short_lo[0].assign((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) {
      short_lo[0][g] = (int)short_t[0].size();
      Index r = cut[g];
      while (r < cut[g + 1]) {
        if (is_long(r)) {
          const int li = long_id[r];
          const Index e = m0[(size_t)r + 1];
          for (Index s0 = m0[r]; s0 < e; s0 += kWaveTile)
            long_t[0].push_back(SpmvBlock{r, r + 1, s0, s0 + kWaveTile < e ? s0 + kWaveTile : e, next_slot[li]++});
          ++r;
          continue;
        }
        const Index start = r;
        Index nnz = 0;
        while (r < cut[g + 1] && r - start < kWaveRows && !is_long(r)) {
          const Index l = m0[(size_t)r + 1] - m0[r];
          if (nnz + l > kWaveTile) break;
          nnz += l;
          ++r;
        }
        short_t[0].push_back(SpmvBlock{start, r, m0[start], m0[r], -1});
      }
    }
    short_lo[0][G] = (int)short_t[0].size();
  }
  for (int b = 1; b < k; ++b) {
    short_lo[b].assign((size_t)G + 1, 0);
    unsigned int p = band_first[b - 1];
    const unsigned int pe = band_first[b];
    for (int g = 0; g < G; ++g) {
      short_lo[b][g] = (int)short_t[b].size();
      while (p < pe && prow[p] < cut[g + 1]) {
        if (long_id[prow[p]] >= 0) {
          const int li = long_id[prow[p]];
          const Index e = pptr[(size_t)p + 1];
          for (Index s0 = pptr[p]; s0 < e; s0 += kWaveTile)
            long_t[b].push_back(SpmvBlock{(int)p, (int)p + 1, s0, s0 + kWaveTile < e ? s0 + kWaveTile : e, next_slot[li]++});
          ++p;
          continue;
        }
        const unsigned int start = p;
        Index nnz = 0;
        while (p < pe && prow[p] < cut[g + 1] && p - start < (unsigned int)kWaveRows && long_id[prow[p]] < 0) {
          const Index l = pptr[(size_t)p + 1] - pptr[p];
          if (nnz + l > kWaveTile) break;
          nnz += l;
          ++p;
        }
        short_t[b].push_back(SpmvBlock{(int)start, (int)p, pptr[start], pptr[p], -1});
      }
    }
    short_lo[b][G] = (int)short_t[b].size();
    if (p != pe) return GRB_PANIC;
  }

  // ---- upload
  auto upload = [&](const void* h, size_t bytes) -> void* {
    void* d = dalloc(bytes, true);
    if (d && bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
  };
  BandArgs& A = B->args;
  A.k = k;
  A.grid = G;
  A.row_cut = (const Index*)upload(cut.data(), 4 * cut.size());
  if (!A.row_cut) return GRB_OUT_OF_MEMORY;
  for (int b = 0; b < k; ++b) {
    BandPhase& P = A.ph[b];
    P.short_tiles = (const SpmvBlock*)upload(short_t[b].data(), sizeof(SpmvBlock) * short_t[b].size());
    P.short_lo = (const int*)upload(short_lo[b].data(), 4 * short_lo[b].size());
    P.long_tiles = (const SpmvBlock*)upload(long_t[b].data(), sizeof(SpmvBlock) * long_t[b].size());
    P.nlong_tiles = (int)long_t[b].size();
    if (!P.short_tiles || !P.short_lo || !P.long_tiles) return GRB_OUT_OF_MEMORY;
    P.ptr = b == 0 ? (const Index*)cnt0 : piece_ptr;
    P.rowmap = b == 0 ? nullptr : piece_row;
    P.ind = b == 0 ? m0_ind : bs_ind;
    P.val = b == 0 ? (const void*)m0_val : (const void*)bs_val;
    P.hot_base = (Index)b * kHot;
    const Index left = plan.npacked - P.hot_base;
    P.nhot = (int)(left < kHot ? (left > 0 ? left : 0) : kHot);
  }
  B->nlong = (int)long_row.size();
  if (B->nlong) {
    B->d_long_row = (int*)upload(long_row.data(), 4 * long_row.size());
    B->d_long_slot_ptr = (int*)upload(slot_ptr.data(), 4 * slot_ptr.size());
    B->d_partials = dalloc(4 * (size_t)slot_ptr.back(), true);
    if (!B->d_long_row || !B->d_long_slot_ptr || !B->d_partials) return GRB_OUT_OF_MEMORY;
  }
  B->d_t = dalloc(4 * (size_t)n, true);
  if (!B->d_t) return GRB_OUT_OF_MEMORY;
  B->band_nnz = nnzb;
  B->pieces = npieces;
  plan.bands = B;
  guard.b = nullptr;
  return GRB_SUCCESS;
}

static grb_info prepare_hub_packing(const CsrArrays& M, SpmvPlan& plan, const Index* other_ptr) {
  plan.hub_ready = true;
  const Index m = plan.nminor;
  plan.nhot = m < kHot ? m : kHot;      // a short vector fits LDS whole: no renaming needed
  if (m <= kHot || M.nvals == 0) return GRB_SUCCESS;
  // columns ranked by reference count on the device (build.hip): counts = row lengths of the transposed
  // orientation when the matrix has one, radix sort by descending count, ties in column order
  Index* d_rank = nullptr;
  GRB_HIP_TRY(hipMalloc(&d_rank, 4 * (size_t)m));
  GRB_HIP_TRY(hipMalloc(&plan.d_order, 4 * (size_t)m));
  long long hot_refs = 0;
  Index nref = 0;
  grb_info ri = device_rank_columns(M.ind, M.nvals, other_ptr, m, kHot, plan.d_order, d_rank, &hot_refs, &nref);
  // worth it only when the LDS prefix takes a real share of the gathers
  if (ri != GRB_SUCCESS || hot_refs * 8 < (long long)M.nvals) {   // < 12.5 %: keep the natural column order
    (void)hipFree(d_rank);
    (void)hipFree(plan.d_order);
    plan.d_order = nullptr;
    plan.nhot = 0;
    return ri;
  }
  // columns nobody references sort last and are never gathered: they need no packing
  plan.npacked = nref;
  GRB_HIP_TRY(hipMalloc(&plan.d_u2, 4 * (size_t)m));
  (void)hipFree(d_rank);
  return GRB_SUCCESS;
}

// rank[order[i]] = i on the device (columns nobody references keep rank 0: they are never looked up)
static grb_info column_ranks(const SpmvPlan& plan, Index** d_rank) {
  const Index m = plan.nminor;
  GRB_HIP_TRY(hipMalloc(d_rank, 4 * (size_t)m));
  GRB_HIP_TRY(hipMemsetAsync(*d_rank, 0, 4 * (size_t)m, ctx().stream));
  hipLaunchKernelGGL(cband_invert_kernel, dim3(ceil_div(plan.npacked, kBlock)), dim3(kBlock), 0, ctx().stream,
                     (const Index*)plan.d_order, plan.npacked, *d_rank);
  GRB_HIP_TRY(hipGetLastError());
  return GRB_SUCCESS;
}

// The CSR kernel's private copy of the column ids renamed by rank (and the optional column bands), made when that
// kernel first runs on a hub-packed orientation -- the column-sorted format below has its own coded copy.
static grb_info ensure_renamed_columns(const CsrArrays& M, SpmvPlan& plan) {
  if (!plan.d_order || plan.d_ind2 || plan.bands) return GRB_SUCCESS;
  Index* d_rank = nullptr;
  GRB_TRY(column_ranks(plan, &d_rank));
  GRB_HIP_TRY(hipMalloc(&plan.d_ind2, 4 * (size_t)M.nvals));
  hipLaunchKernelGGL(rename_columns_kernel, dim3(stream_grid(M.nvals, kBlock)), dim3(kBlock), 0, ctx().stream,
                     M.ind, M.nvals, d_rank, plan.d_ind2);
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  // column bands: more LDS prefixes when the columns after the first still carry weight
  const grb_info bi = prepare_bands(M, plan, d_rank);
  (void)hipFree(d_rank);
  if (bi == GRB_SUCCESS && plan.bands) {                    // the banded copy replaces the renamed column ids
    (void)hipFree(plan.d_ind2);
    plan.d_ind2 = nullptr;
  }
  return bi == GRB_OUT_OF_MEMORY ? GRB_SUCCESS : bi;        // no room for the second copy: one prefix it is
}

// ---- column-sorted row bands (spmv_cband.hpp): preparation -----------------------------------------------------
// 0 = CSR kernel only, 1 = auto (the column-sorted format on hub-packed orientations, commutative monoids),
// 2 = the column-sorted format wherever the monoid allows it (tests).  GRB_SPMV_FORMAT=csr|auto|cband.
static int g_spmv_format = -1;
int spmv_format_setting(int set) {
  if (g_spmv_format < 0) {
    const char* e = getenv("GRB_SPMV_FORMAT");
    g_spmv_format = !e ? 1 : (!strcmp(e, "csr") ? 0 : (!strcmp(e, "cband") ? 2 : 1));
  }
  if (set >= 0) g_spmv_format = set > 2 ? 2 : set;
  return g_spmv_format;
}

// `auto` takes the column-sorted format for an orientation once that orientation has run this many products through
// the CSR kernel (GRB_SPMV_CBAND_AFTER, grb_spmv_set_reuse_threshold; 0 = at the first product).  Preparing the format
// costs about 70 CSR-kernel launches' worth of the time it then saves per launch (RMAT-22: 20 ms against 0.3 ms), so
// a matrix that is multiplied a few dozen times and dropped -- a 20-iteration PageRank -- never pays it, and a matrix
// that keeps being multiplied pays it once, at most doubling what the format would have cost from the start
// (the rent-or-buy rule).
static int g_cband_after = -1;
int spmv_reuse_threshold(int set) {
  if (g_cband_after < 0) g_cband_after = getenv("GRB_SPMV_CBAND_AFTER") ? atoi(getenv("GRB_SPMV_CBAND_AFTER")) : 48;
  const int before = g_cband_after;
  if (set >= 0) g_cband_after = set;
  return before;
}

static int cband_bits_for(long long dim) {
  int b = 1;
  while (b < 32 && (1ll << b) < dim) ++b;
  return b;
}

static grb_info prepare_cband(const CsrArrays& M, SpmvPlan& plan) {
  plan.cband_tried = true;
  const Index n = plan.nrows;
  const long long nnz = M.nvals;
  if (n <= 0 || nnz <= 0) return GRB_SUCCESS;
  hipStream_t st = ctx().stream;
  const int G = ctx().num_cu * kCbWgPerCu;
  SpmvCBand* C = new SpmvCBand();
  struct Guard { SpmvCBand* c; ~Guard() { free_spmv_cband(c); } } guard{C};
  std::vector<void*> temp;
  struct TempGuard { std::vector<void*>& v; ~TempGuard() { for (void* p : v) if (p) (void)hipFree(p); } } tguard{temp};
  bool oom = false;
  auto dalloc = [&](size_t bytes, bool keep) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) { (void)hipGetLastError(); oom = true; return nullptr; }
    (keep ? C->owned : temp).push_back(p);
    return p;
  };
  auto upload = [&](const void* h, size_t bytes, bool keep) -> void* {
    void* d = dalloc(bytes, keep);
    if (d && bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) { oom = true; return nullptr; }
    return d;
  };

  // GRB_SPMV_PREP_TRACE: where the preparation's time goes (stderr; every mark waits for the stream)
  static const bool prep_trace = getenv("GRB_SPMV_PREP_TRACE") != nullptr;
  auto t_prev = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (!prep_trace) return;
    (void)hipStreamSynchronize(st);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "cband prep: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
    t_prev = now;
  };
  // ---- hubs, bands, every row's place: on the device (spmv_cband.hpp); GRB_CB_PREP_HOST=1 keeps the host pass of rounds
  // 3-5 (same tables: the tests run both), which is also where the two cases the device pass does not cover end up
  static const bool host_pass_wanted = getenv("GRB_CB_PREP_HOST") != nullptr && atoi(getenv("GRB_CB_PREP_HOST")) != 0;
  static const int light_weight = getenv("GRB_CB_LIGHT_WEIGHT") ? atoi(getenv("GRB_CB_LIGHT_WEIGHT")) : 14;   // hub = 10
  std::vector<CbBand> bands;
  std::vector<long long> band_start;                     // sorted position of every band's first entry
  int nhub = 0;
  unsigned int* d_row_band = nullptr;
  unsigned short* d_row_loc = nullptr;
  Index* d_hub_rows = nullptr;
  unsigned int* d_hub_bits = nullptr;
  // Light bands are sized so that a whole number of them is one workgroup's share: the hub band gets the
  // workgroups its cost asks for (a light entry costs more than a hub entry, see the dealing below), the light
  // rows' entries are split evenly over the rest, and a share that does not fit kCbRows rows is cut into k equal
  // bands -- then the equal-cost cuts of the dealing fall on band boundaries and few bands need partial slices.
  auto light_band_limit = [&](long long hub_entries, int nh) -> long long {
    long long band_entries_max = (long long)kCbLightGroups * kWave;
    const long long light_entries = nnz - hub_entries;
    const double hub_cost = 10.0 * (double)hub_entries, light_cost = (double)light_weight * (double)light_entries;
    int wg_hub = nh > 0 ? (int)(G * hub_cost / (hub_cost + light_cost) + 0.5) : 0;
    if (nh > 0 && wg_hub < 1) wg_hub = 1;
    if (wg_hub > G - 1) wg_hub = G - 1;
    const long long share = light_entries / (G - wg_hub) + 1;                 // entries per light workgroup
    const double rows_per_share = (double)share * (double)(n - nh) / (double)(light_entries > 0 ? light_entries : 1);
    const int k = (int)(rows_per_share / (0.97 * kCbRows)) + 1;
    if (share / k + 1 < band_entries_max) band_entries_max = share / k + 1;
    if (band_entries_max < 64 * kWave) band_entries_max = 64 * kWave;
    return band_entries_max;
  };
  bool host_pass = host_pass_wanted;
  if (!host_pass) {
    constexpr int kBandCap = 1 << 20;
    unsigned int* d_hist = (unsigned int*)dalloc(4 * ((size_t)kCbDegBins + 1), false);
    unsigned int* d_light = (unsigned int*)dalloc(4 * ((size_t)n + 1), false);
    unsigned int* d_flag = (unsigned int*)dalloc(4 * ((size_t)n + 1), false);
    Index* d_next = (Index*)dalloc(4 * (size_t)n, false);
    Index* d_starts = (Index*)dalloc(4 * ((size_t)kBandCap + 1), false);
    int* d_count = (int*)dalloc(16, false);
    d_row_band = (unsigned int*)dalloc(4 * (size_t)n, false);
    d_row_loc = (unsigned short*)dalloc(2 * (size_t)n, false);
    d_hub_bits = (unsigned int*)dalloc(4 * (((size_t)n + 31) / 32), true);
    if (oom) return GRB_OUT_OF_MEMORY;
    Index hub_above = 0x7fffffff;                          // rows with more entries than this are hubs
    if (n > kCbRows) {
      GRB_HIP_TRY(hipMemsetAsync(d_hist, 0, 4 * ((size_t)kCbDegBins + 1), st));
      hipLaunchKernelGGL(cband_degree_hist_kernel, dim3(G), dim3(1024), 0, st, M.ptr, n, d_hist);
      GRB_HIP_TRY(hipGetLastError());
      std::vector<unsigned int> hist((size_t)kCbDegBins + 1);
      GRB_HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, 4 * hist.size(), hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipStreamSynchronize(st));
      long long above = hist[kCbDegBins];
      if (above > kCbRows) {
        host_pass = true;                                  // the threshold lies among rows of >= 65 536 entries: selected on the host
      } else {
        int d = kCbDegBins - 1;
        for (; d > 0; --d) {                               // the largest d with (rows of degree >= d) >= kCbRows + 1
          above += hist[d];
          if (above > kCbRows) break;
        }
        hub_above = d;
        if (hub_above < 64) hub_above = 64;                // at most kCbRows rows are strictly above the (kCbRows+1)-th largest
      }
    }
    mark("degree histogram + hub threshold");
    if (!host_pass) {
      hipLaunchKernelGGL(cband_light_kernel, dim3(stream_grid((long long)n + kWave, kBlock)), dim3(kBlock), 0, st, M.ptr, n, hub_above,
                         d_light, d_flag, d_hub_bits);
      GRB_HIP_TRY(hipGetLastError());
      GRB_TRY(device_exclusive_scan_u32(d_light, (long long)n + 1));
      GRB_TRY(device_exclusive_scan_u32(d_flag, (long long)n + 1));
      unsigned int tot[2] = {0u, 0u};                      // light entries, hubs
      GRB_HIP_TRY(hipMemcpyAsync(&tot[0], d_light + n, 4, hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipMemcpyAsync(&tot[1], d_flag + n, 4, hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipStreamSynchronize(st));
      nhub = (int)tot[1];
      const long long hub_entries = nnz - (long long)tot[0];
      const long long band_entries_max = light_band_limit(hub_entries, nhub);
      hipLaunchKernelGGL(cband_next_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, (const unsigned int*)d_light, n,
                         (unsigned int)band_entries_max, kCbRows, d_next);
      hipLaunchKernelGGL(cband_chase_kernel, dim3(1), dim3(64), 0, st, (const Index*)d_next, n, d_starts, kBandCap, d_count);
      GRB_HIP_TRY(hipGetLastError());
      int nlight = 0;
      GRB_HIP_TRY(hipMemcpyAsync(&nlight, d_count, 4, hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipStreamSynchronize(st));
      if (nlight > kBandCap) return GRB_SUCCESS;           // a million bands: not a matrix for this format
      d_hub_rows = (Index*)dalloc(4 * (size_t)(nhub > 0 ? nhub : 1), true);
      long long* d_first = (long long*)dalloc(8 * ((size_t)nlight + 1), false);
      if (oom) return GRB_OUT_OF_MEMORY;
      const unsigned int band0 = nhub > 0 ? 1u : 0u;
      hipLaunchKernelGGL(cband_place_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, (const Index*)d_starts, nlight, band0,
                         (const unsigned int*)d_light, (const unsigned int*)d_flag, (const unsigned int*)d_hub_bits, n,
                         (unsigned long long)hub_entries, d_row_band, d_row_loc, d_hub_rows, d_first);
      GRB_HIP_TRY(hipGetLastError());
      std::vector<Index> starts((size_t)nlight + 1);
      std::vector<long long> first((size_t)nlight);
      GRB_HIP_TRY(hipMemcpyAsync(starts.data(), d_starts, 4 * starts.size(), hipMemcpyDeviceToHost, st));
      if (nlight > 0) GRB_HIP_TRY(hipMemcpyAsync(first.data(), d_first, 8 * first.size(), hipMemcpyDeviceToHost, st));
      GRB_HIP_TRY(hipStreamSynchronize(st));
      if (nhub > 0) {
        bands.push_back(CbBand{0, nhub, 1});
        band_start.push_back(0);
      }
      for (int b = 0; b < nlight; ++b) {
        bands.push_back(CbBand{starts[b], starts[(size_t)b + 1] - starts[b], 0});
        band_start.push_back(first[b]);
      }
      band_start.push_back(nnz);
    }
  }
  if (host_pass) {
    // ---- host: hubs, bands
    std::vector<Index> ptr((size_t)n + 1);
    GRB_HIP_TRY(hipMemcpy(ptr.data(), M.ptr, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost));
    Index hub_above = 0x7fffffff;                          // rows with more entries than this are hubs
    if (n > kCbRows) {
      // the (kCbRows + 1)-th largest degree, from a histogram (one pass over the rows; degrees of 64 Ki and more share
      // the last bin -- should the answer fall there, the selection is done on those rows alone)
      constexpr int kDegBins = 65536;
      std::vector<unsigned int> hist((size_t)kDegBins + 1, 0u);
      for (Index r = 0; r < n; ++r) {
        const Index d = ptr[(size_t)r + 1] - ptr[r];
        ++hist[d < kDegBins ? d : kDegBins];
      }
      long long above = hist[kDegBins];
      if (above > kCbRows) {
        std::vector<Index> deg;
        for (Index r = 0; r < n; ++r)
          if (ptr[(size_t)r + 1] - ptr[r] >= kDegBins) deg.push_back(ptr[(size_t)r + 1] - ptr[r]);
        std::nth_element(deg.begin(), deg.begin() + kCbRows, deg.end(), [](Index x, Index y) { return x > y; });
        hub_above = deg[kCbRows];
      } else {
        int d = kDegBins - 1;
        for (; d > 0; --d) {                                 // the largest d with (rows of degree >= d) >= kCbRows + 1
          above += hist[d];
          if (above > kCbRows) break;
        }
        hub_above = d;
      }
      if (hub_above < 64) hub_above = 64;                    // at most kCbRows rows are strictly above the (kCbRows+1)-th largest
    }
    mark("row pointers + hub threshold");
    std::vector<unsigned int> row_band((size_t)n);
    std::vector<unsigned short> row_loc((size_t)n);
    std::vector<Index> hub_rows;
    std::vector<unsigned int> hub_bits(((size_t)n + 31) / 32, 0u);
    long long hub_entries = 0;
    for (Index r = 0; r < n; ++r)
      if (ptr[(size_t)r + 1] - ptr[r] > hub_above) {
        hub_bits[r >> 5] |= 1u << (r & 31);
        hub_rows.push_back(r);
        hub_entries += ptr[(size_t)r + 1] - ptr[r];
      }
    const int nhub_h = (int)hub_rows.size();
    bands.clear();
    band_start.clear();
    if (nhub_h > 0) {
      bands.push_back(CbBand{0, nhub_h, 1});
      band_start.push_back(0);
    }
    const long long band_entries_max = light_band_limit(hub_entries, nhub_h);
    {
      // one pass over the rows: the light bands are cut, and every row learns its band and its place in it
      long long at = hub_entries, in_band = 0;
      Index r0 = 0;
      int hub_i = 0;
      unsigned int cur_band = (unsigned int)bands.size();   // the band being filled
      for (Index r = 0; r < n; ++r) {
        const bool hub = (hub_bits[r >> 5] >> (r & 31)) & 1u;
        const Index d = hub ? 0 : ptr[(size_t)r + 1] - ptr[r];
        if (r > r0 && (r - r0 == kCbRows || in_band + d > band_entries_max)) {
          bands.push_back(CbBand{r0, r - r0, 0});
          band_start.push_back(at);
          at += in_band;
          in_band = 0;
          r0 = r;
          ++cur_band;
        }
        in_band += d;
        row_band[r] = hub ? 0u : cur_band;
        row_loc[r] = (unsigned short)(hub ? hub_i++ : r - r0);
      }
      bands.push_back(CbBand{r0, n - r0, 0});
      band_start.push_back(at);
      at += in_band;
      band_start.push_back(at);
      if (at != nnz) return GRB_PANIC;
    }

    nhub = nhub_h;
    d_row_band = (unsigned int*)upload(row_band.data(), 4 * (size_t)n, false);
    d_row_loc = (unsigned short*)upload(row_loc.data(), 2 * (size_t)n, false);
    d_hub_rows = (Index*)upload(hub_rows.data(), 4 * hub_rows.size(), true);
    if (d_hub_bits) GRB_HIP_TRY(hipMemcpy(d_hub_bits, hub_bits.data(), 4 * hub_bits.size(), hipMemcpyHostToDevice));
    else d_hub_bits = (unsigned int*)upload(hub_bits.data(), 4 * hub_bits.size(), true);
    if (oom) return GRB_OUT_OF_MEMORY;
  }
  const int nbands = (int)bands.size();
  mark("bands (host pass)");

  // ---- device: keys, sort, segments
  // column codes: the hot prefix of the rank order (<= 512 Ki columns, packed per launch: 6 MB instead of the whole
  // vector's 50), then every column under its own id -- past the prefix a band's list is as sparse in rank order
  // as in natural order, so packing the tail buys no locality
  unsigned int nhot = 0;
  Index* d_rank = nullptr;
  const Index* d_ind2 = nullptr;                           // the CSR kernel's renamed column ids, when it has run already
  if (plan.d_order) {
    const unsigned int want = ((unsigned int)plan.npacked + 65535u) & ~65535u;
    nhot = want < 8u * 65536u ? want : 8u * 65536u;
    if (plan.d_ind2) {
      d_ind2 = plan.d_ind2;                                // rank < nhot ? rank : nhot + column, formed per entry: no gather
    } else {
      GRB_TRY(column_ranks(plan, &d_rank));
      temp.push_back(d_rank);
      hipLaunchKernelGGL(cband_codes_kernel, dim3(ceil_div(plan.nminor, kBlock)), dim3(kBlock), 0, st, d_rank, plan.nminor, nhot);
      GRB_HIP_TRY(hipGetLastError());
    }
  }
  const long long ncols = (long long)nhot + (long long)plan.nminor;
  unsigned long long* d_keys = (unsigned long long*)dalloc(8 * (size_t)nnz, false);
  unsigned int* d_pay = (unsigned int*)dalloc(4 * (size_t)nnz, false);
  if (oom) return GRB_OUT_OF_MEMORY;
  // key = ((band << colbits | column code) << 16) | row in band; sorted on the bits above the low 16 only
  // (the column field also has to hold the end of the last 65536-column block: the segment search compares against it)
  const long long col_span = ((ncols + 65535) / 65536) << 16;
  const int colbits = cband_bits_for(col_span > ncols ? col_span : ncols), bandbits = cband_bits_for(nbands);
  if (colbits + bandbits + kCbKeyLow > 64) return GRB_SUCCESS;
  mark("ranks, uploads, allocations");
  hipLaunchKernelGGL(cband_keys_kernel, dim3(stream_grid((long long)n, kBlock)), dim3(kBlock), 0, st, M.ptr, M.ind,
                     (const unsigned int*)M.val, n, (const unsigned int*)d_row_band, (const unsigned short*)d_row_loc,
                     (const unsigned int*)d_hub_bits, (const Index*)d_rank, d_ind2, nhot, colbits, d_keys, d_pay);
  if (nhub > 0)
    hipLaunchKernelGGL(cband_keys_hub_kernel, dim3(nhub < 4096 ? nhub : 4096), dim3(1024), 0, st, M.ptr, M.ind,
                       (const unsigned int*)M.val, (const Index*)d_hub_rows, nhub, (const Index*)d_rank, d_ind2, nhot, colbits,
                       d_keys, d_pay);
  GRB_HIP_TRY(hipGetLastError());
  {
    const grb_info si = device_sort_pairs_range(d_keys, d_pay, nnz, kCbKeyLow, colbits + bandbits);
    if (si != GRB_SUCCESS) return si == GRB_PANIC ? GRB_OUT_OF_MEMORY : si;     // the sort's scratch did not fit
  }
  mark("keys + sort");
  const int ncb = (int)((ncols + 65535) / 65536);
  long long* d_band_start = (long long*)upload(band_start.data(), 8 * band_start.size(), false);
  long long* d_seg = (long long*)dalloc(8 * (size_t)nbands * (size_t)(ncb + 1), false);
  if (oom) return GRB_OUT_OF_MEMORY;
  hipLaunchKernelGGL(cband_segments_kernel, dim3(ceil_div((long long)nbands * (ncb + 1), kBlock)), dim3(kBlock), 0, st,
                     (const unsigned long long*)d_keys, (const long long*)d_band_start, nbands, ncb, colbits, d_seg);
  GRB_HIP_TRY(hipGetLastError());
  std::vector<long long> seg((size_t)nbands * (size_t)(ncb + 1));
  GRB_HIP_TRY(hipMemcpy(seg.data(), d_seg, 8 * seg.size(), hipMemcpyDeviceToHost));

  // ---- host: non-empty segments -> groups; the bands' group ranges
  std::vector<long long> seg_entry, seg_group, seg_band_g0;
  std::vector<unsigned int> seg_base;
  std::vector<long long> band_g((size_t)nbands + 1, 0);
  long long ngroups = 0;
  for (int b = 0; b < nbands; ++b) {
    band_g[b] = ngroups;
    for (int cb = 0; cb < ncb; ++cb) {
      const long long e0 = seg[(size_t)b * (ncb + 1) + cb], e1 = seg[(size_t)b * (ncb + 1) + cb + 1];
      if (e1 <= e0) continue;
      seg_entry.push_back(e0);
      seg_group.push_back(ngroups);
      seg_base.push_back((unsigned int)cb << 16);
      seg_band_g0.push_back(band_g[b]);
      ngroups += (e1 - e0 + kWave - 1) / kWave;
    }
    ngroups = band_g[b] + (ngroups - band_g[b] + kCbChunk - 1) / kCbChunk * kCbChunk;   // whole chunks: the tail is padding
  }
  band_g[nbands] = ngroups;
  const int nseg = (int)seg_entry.size();
  if (nseg == 0 || ngroups <= 0 || ngroups >= (1ll << 31)) return GRB_SUCCESS;
  seg_entry.push_back(nnz);                               // closes the last segment (segments tile [0, nnz))
  seg_group.push_back(ngroups);
  // a segment ends where the next begins, except across bands with empty tails: make the ends explicit
  std::vector<long long> seg_end_fix = seg_entry;
  {
    int si = 0;
    for (int b = 0; b < nbands; ++b)
      for (int cb = 0; cb < ncb; ++cb) {
        const long long e0 = seg[(size_t)b * (ncb + 1) + cb], e1 = seg[(size_t)b * (ncb + 1) + cb + 1];
        if (e1 <= e0) continue;
        if (seg_end_fix[(size_t)si + 1] != e1) return GRB_PANIC;   // sorted keys tile the range: cannot happen
        ++si;
      }
  }

  mark("segments (device + host)");
  // ---- iso?
  unsigned int iso_out[2] = {0xffffffffu, 0u};
  if (M.val) {
    unsigned int* d_iso = (unsigned int*)upload(iso_out, 8, false);
    if (oom) return GRB_OUT_OF_MEMORY;
    hipLaunchKernelGGL(cband_iso_kernel, dim3(stream_grid(nnz, kBlock * 8)), dim3(kBlock), 0, st, (const unsigned int*)M.val, nnz,
                       d_iso);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpy(iso_out, d_iso, 8, hipMemcpyDeviceToHost));
  } else {
    return GRB_SUCCESS;                                   // a matrix without a value array never reaches the generic SpMV
  }
  C->iso = iso_out[0] == iso_out[1];

  mark("iso test");
  // ---- device: the coded entries
  long long* d_seg_entry = (long long*)upload(seg_entry.data(), 8 * seg_entry.size(), false);
  long long* d_seg_group = (long long*)upload(seg_group.data(), 8 * seg_group.size(), false);
  long long* d_seg_band_g0 = (long long*)upload(seg_band_g0.data(), 8 * seg_band_g0.size(), false);
  unsigned int* d_seg_base = (unsigned int*)upload(seg_base.data(), 4 * seg_base.size(), false);
  // (a wave step reads whole 4-group chunks: room for the last chunk to run past the last group)
  unsigned int* d_pack = (unsigned int*)dalloc(4 * (size_t)(ngroups + kCbChunk) * kWave, true);
  unsigned int* d_val2 = C->iso ? nullptr : (unsigned int*)dalloc(4 * (size_t)(ngroups + kCbChunk) * kWave, true);
  unsigned int* d_gbase = (unsigned int*)dalloc(4 * (size_t)ngroups, true);
  if (oom) return GRB_OUT_OF_MEMORY;
  hipLaunchKernelGGL(cband_emit_kernel, dim3(stream_grid(ngroups * kWave, kBlock)), dim3(kBlock), 0, st,
                     (const unsigned long long*)d_keys, (const unsigned int*)d_pay, (const long long*)d_seg_entry,
                     (const long long*)d_seg_group, (const unsigned int*)d_seg_base, (const long long*)d_seg_band_g0, nseg, ngroups,
                     colbits, d_pack, d_val2, d_gbase);
  GRB_HIP_TRY(hipGetLastError());

  mark("emit");
  // ---- items: the bands' groups form one sequence (hub band first); it is cut into one piece of equal COST per
  // workgroup -- a light band's group costs more than the hub band's: its column-sorted list is sparser, so its
  // gathers touch more lines (GRB_SPMV_TRACE, ticks per group per workgroup: 3.3 against 2.0) -- so every
  // workgroup walks consecutive groups (consecutive columns) and at most its first and last band are shared with
  // a neighbour.  A band that several workgroups share is accumulated in partial slices, folded by the second kernel.
  auto weight = [&](int b) { return (long long)(bands[b].hub ? 10 : light_weight); };
  auto fixed = [&](int b) { return (long long)bands[b].nrows / 4 + 40; };        // clearing and writing the slice
  long long total_cost = 0;
  for (int b = 0; b < nbands; ++b) total_cost += (band_g[b + 1] - band_g[b]) * weight(b) + fixed(b);
  std::vector<CbItem> dealt;
  std::vector<int> item_wg;
  std::vector<int> wg_ptr((size_t)G + 1, 0);
  // one pass of the cutting for a given share; returns the largest load any workgroup ends up with
  auto deal = [&](long long target) -> long long {
    dealt.clear();
    item_wg.clear();
    int wg = 0;
    long long acc = 0, worst = 0;
    for (int b = 0; b < nbands; ++b) {
      long long g = band_g[b];
      const long long band_cost = (band_g[b + 1] - g) * weight(b) + fixed(b);
      if (g == band_g[b + 1]) {                            // no entries: a light band still writes its rows
        if (!bands[b].hub) { dealt.push_back(CbItem{b, (int)g, (int)g, -1}); item_wg.push_back(wg); acc += fixed(b); }
        continue;
      }
      // a band that nearly fits is not started here, one that nearly ends is finished here: whole bands where possible
      const long long slack = (band_cost < target ? band_cost : target) / 6;
      if (wg < G - 1 && acc > 0 && target - acc < band_cost && target - acc < slack) { worst = acc > worst ? acc : worst; ++wg; acc = 0; }
      while (g < band_g[b + 1]) {
        long long take = band_g[b + 1] - g;
        if (wg < G - 1) {
          long long room = (target - acc - fixed(b)) / weight(b);
          room = room / kCbChunk * kCbChunk;
          if (room < kCbChunk) room = kCbChunk;
          if (room < take && (take - room) * weight(b) > slack) take = room;
        }
        dealt.push_back(CbItem{b, (int)g, (int)(g + take), -1});
        item_wg.push_back(wg);
        acc += take * weight(b) + fixed(b);
        g += take;
        if (acc >= target && wg < G - 1) { worst = acc > worst ? acc : worst; ++wg; acc = 0; }
      }
    }
    return acc > worst ? acc : worst;
  };
  // the per-item fixed costs and the snapping are not in total_cost / G: try shares up to 1.6 x that, keep the best
  {
    const long long base = total_cost / G + 1;
    long long best_target = base, best = -1;
    for (int k = 0; k <= 60; ++k) {
      const long long t = base + base * k / 100;
      const long long worst = deal(t);
      if (best < 0 || worst < best) { best = worst; best_target = t; }
    }
    (void)deal(best_target);
  }
  {
    size_t i = 0;
    C->wg_groups.clear(); C->wg_hub_groups.clear(); C->wg_items.clear();
    for (int g = 0; g < G; ++g) {
      wg_ptr[g] = (int)i;
      int gr = 0, hg = 0, ni = 0;
      while (i < dealt.size() && item_wg[i] == g) {
        gr += dealt[i].g1 - dealt[i].g0;
        if (bands[dealt[i].band].hub) hg += dealt[i].g1 - dealt[i].g0;
        ++ni; ++i;
      }
      C->wg_groups.push_back(gr); C->wg_hub_groups.push_back(hg); C->wg_items.push_back(ni);
    }
    wg_ptr[G] = (int)dealt.size();
  }
  // partial slices for the bands more than one workgroup works on
  std::vector<int> fin_band, fin_ptr(1, 0), fin_off;
  long long partial_elems = 0;
  int max_fin_rows = 0;
  for (size_t i = 0; i < dealt.size();) {
    size_t j = i;
    while (j < dealt.size() && dealt[j].band == dealt[i].band) ++j;
    if (j - i > 1) {
      const int b = dealt[i].band;
      fin_band.push_back(b);
      for (size_t k = i; k < j; ++k) {
        dealt[k].slot_off = (int)partial_elems;
        fin_off.push_back((int)partial_elems);
        partial_elems += bands[b].nrows;
      }
      fin_ptr.push_back((int)fin_off.size());
      if (bands[b].nrows > max_fin_rows) max_fin_rows = bands[b].nrows;
    }
    i = j;
  }
  if (partial_elems >= (1ll << 31)) return GRB_SUCCESS;
  const int nslots = (int)fin_off.size();

  mark("dealing (host)");
  CbArgs& A = C->args;
  A.bands = (const CbBand*)upload(bands.data(), sizeof(CbBand) * bands.size(), true);
  A.items = (const CbItem*)upload(dealt.data(), sizeof(CbItem) * dealt.size(), true);
  A.wg_ptr = (const int*)upload(wg_ptr.data(), 4 * wg_ptr.size(), true);
  A.fin_band = (const int*)upload(fin_band.data(), 4 * fin_band.size(), true);
  A.fin_ptr = (const int*)upload(fin_ptr.data(), 4 * fin_ptr.size(), true);
  A.fin_off = (const int*)upload(fin_off.data(), 4 * fin_off.size(), true);
  A.pack = d_pack;
  A.val = d_val2;
  A.gbase = d_gbase;
  A.hub_rows = d_hub_rows;
  A.hub_bits = d_hub_bits;
  A.iso_bits = iso_out[0];
  A.nhub = nhub;
  if (partial_elems > 0) C->d_partials = dalloc(8 * (size_t)partial_elems, true);   // accumulators of <= 8 bytes
  C->nfin = (int)fin_band.size();
  C->max_fin_rows = max_fin_rows;
  C->partial_elems = partial_elems;
  if (oom) return GRB_OUT_OF_MEMORY;
  GRB_HIP_TRY(hipStreamSynchronize(st));
  mark("uploads of the tables");
  C->grid = G;
  C->nhot = nhot;
  C->nbands = nbands;
  C->nitems = (int)dealt.size();
  C->nslots = nslots;
  C->ngroups = ngroups;
  C->entries = nnz;
  plan.cband = C;
  guard.c = nullptr;
  return GRB_SUCCESS;
}

// Epilogue shared by the SpMV kernels: mask -> identity where the mask FAILS
// (spmv.hpp:203-212), then optional accumulate with the semiring's add (:213-220).
template <int SR, typename T>
__device__ inline void spmv_store(T* w, Index row, T value, const void* mask, int mask_f32, int scmp,
                                  int accum) {
  typedef Semiring<SR, T> S;
  if (mask && !mask_pass(mask, mask_f32, scmp, row)) value = S::identity();
  if (accum) value = S::add(w[row], value);
  w[row] = value;
}

// A matrix without stored entries: every row is the empty sum.
template <int SR, typename T>
__global__ void spmv_empty_kernel(Index n, const void* __restrict__ mask, int mask_f32, int scmp, int accum, T* w) {
  const Index i = (Index)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) spmv_store<SR, T>(w, i, Semiring<SR, T>::identity(), mask, mask_f32, scmp, accum);
}

constexpr int kFinalLanes = 16;   // lanes folding the partials of one long row
template <int SR, typename T>
__global__ void spmv_long_finalize_kernel(const int* __restrict__ long_row, const int* __restrict__ slot_ptr,
                                          int nlong, const T* __restrict__ partials,
                                          const void* __restrict__ mask, int mask_f32, int scmp, int accum,
                                          T* w) {
  typedef Semiring<SR, T> S;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / kFinalLanes, l = t % kFinalLanes;
  T acc = S::identity();
  if (i < nlong)
    for (int s = slot_ptr[i] + l; s < slot_ptr[i + 1]; s += kFinalLanes) acc = S::add(acc, partials[s]);
  acc = group_reduce(acc, kFinalLanes, [](T x, T y) { return S::add(x, y); });
  if (i < nlong && l == 0) spmv_store<SR, T>(w, long_row[i], acc, mask, mask_f32, scmp, accum);
}

// ---- hub-packed kernel ------------------------------------------------------------------
// One persistent 1024-thread workgroup per CU.  The workgroup stages the first `nhot` values
// of the (packed) input vector in LDS once; after that its 16 waves run independently, each
// looping over wave tiles with a private 2 KiB product buffer and no workgroup barrier:
//   stream   8 coalesced (column, value) pairs per lane, non-temporal so the matrix stream does
//            not push the vector out of L2;
//   gather   column < nhot from LDS, the rest from global memory (L2 for the warm tail);
//   reduce   products -> LDS, rows folded with L lanes per row (L adapted to the tile).
// The streaming part is written without branches (clamped indices instead of predicates:
// a lane past the end of its tile re-reads the tile's last element and contributes the
// identity; a lane whose column is hot points its global gather at u[0], which coalesces to
// one request) so that the sixteen stream loads and eight gathers of a tile are issued back to
// back and the tile after it is already in flight while this one is reduced.
template <int SR, typename T>
__global__ __launch_bounds__(kHubThreads) void spmv_hub_kernel(
    const SpmvBlock* __restrict__ tiles, int ntiles, const Index* __restrict__ ptr,
    const Index* __restrict__ ind, const T* __restrict__ val, const T* __restrict__ u, int nhot,
    const void* __restrict__ mask, int mask_f32, int scmp, int accum, T* w, T* __restrict__ partials) {
  typedef Semiring<SR, T> S;
  __shared__ T hot[kHot];
  __shared__ T stage[kHubWaves][kWaveTile];
  const int tid = threadIdx.x;
  for (int i = tid; i < nhot; i += kHubThreads) hot[i] = u[i];
  __syncthreads();
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  T* prod = stage[wave];
  constexpr int kPer = kWaveTile / kWave;
  const int stride = gridDim.x * kHubWaves;
  const int t0 = blockIdx.x * kHubWaves + wave;
  if (t0 >= ntiles) return;
  const int count = (ntiles - t0 + stride - 1) / stride;   // tiles of this wave
  const int t_last = t0 + (count - 1) * stride;
  const int hot_clamp = nhot > 0 ? nhot - 1 : 0;
  auto tile_at = [&](int i) { const int t = t0 + i * stride; return tiles[t < t_last ? t : t_last]; };

  // Three tiles are in flight per wave: tile i is reduced out of registers/LDS while the
  // gathers of tile i+1 and the (column, value, row pointer) stream of tile i+2 are
  // outstanding; the only wait on memory is at the bottom of the loop.
  SpmvBlock b0, b1, b2;          // reduce stage, gather stage, stream stage
  T pr[kPer];                    // products of the reduce-stage tile
  Index rlo0, rhi0;              // its row pointers, lane r holding row r
  Index c1[kPer], rlo1, rhi1;
  T a1[kPer];

#define GRB_HUB_STREAM(B, C, A, RLO, RHI)                                  \
  _Pragma("unroll") for (int k = 0; k < kPer; ++k) {                        \
    int p = (B).nnz_start + lane + k * kWave;                               \
    p = p < (B).nnz_end ? p : (B).nnz_end - 1;                              \
    p = p > 0 ? p : 0;                                                      \
    (C)[k] = stream_load(&ind[p]);                                          \
    (A)[k] = stream_load(&val[p]);                                          \
  }                                                                         \
  {                                                                         \
    const int r = (B).row_start + lane;                                     \
    RLO = ptr[r < (B).row_end ? r : (B).row_end];                           \
    RHI = ptr[r + 1 < (B).row_end ? r + 1 : (B).row_end];                   \
  }
#define GRB_HUB_COLD(C) ((unsigned)(C) >= (unsigned)nhot)
#define GRB_HUB_LDS_INDEX(C) ((C) < hot_clamp ? (C) : hot_clamp)
#define GRB_HUB_GATHER(C, XG, XL)                                                                  \
  _Pragma("unroll") for (int k = 0; k < kPer; ++k) (XG)[k] = u[GRB_HUB_COLD((C)[k]) ? (C)[k] : 0];  \
  _Pragma("unroll") for (int k = 0; k < kPer; ++k) (XL)[k] = hot[GRB_HUB_LDS_INDEX((C)[k])];
#define GRB_HUB_PRODUCTS(B, C, A, XG, XL)                                               \
  _Pragma("unroll") for (int k = 0; k < kPer; ++k) {                                     \
    const T x = GRB_HUB_COLD((C)[k]) ? (XG)[k] : (XL)[k];                                \
    pr[k] = lane + k * kWave < (B).nnz_end - (B).nnz_start ? S::mul((A)[k], x) : S::identity(); \
  }

  b0 = tile_at(0);
  b1 = tile_at(1);
  b2 = tile_at(2);
  {
    Index c0[kPer];
    T a0[kPer], xg[kPer], xl[kPer];
    GRB_HUB_STREAM(b0, c0, a0, rlo0, rhi0)
    GRB_HUB_GATHER(c0, xg, xl)
    asm volatile("" ::: "memory");
    GRB_HUB_STREAM(b1, c1, a1, rlo1, rhi1)
    asm volatile("" ::: "memory");
    GRB_HUB_PRODUCTS(b0, c0, a0, xg, xl)
  }
  for (int i = 0; i < count; ++i) {
    // ---- issue: gathers of tile i+1, stream of tile i+2, descriptor of tile i+3
    T xg[kPer], xl[kPer];
    Index c2[kPer], rlo2, rhi2;
    T a2[kPer];
    GRB_HUB_GATHER(c1, xg, xl)
    asm volatile("" ::: "memory");
    GRB_HUB_STREAM(b2, c2, a2, rlo2, rhi2)
    asm volatile("" ::: "memory");
    const SpmvBlock b3 = tile_at(i + 3);

    // ---- reduce tile i (no global loads in here unless a mask / accumulate is requested)
    const int nnz = b0.nnz_end - b0.nnz_start;
    if (b0.slot >= 0) {                 // slice of a long row: fold in registers
      T acc = pr[0];
#pragma unroll
      for (int k = 1; k < kPer; ++k) acc = S::add(acc, pr[k]);
      acc = wave_reduce(acc, [](T p, T q) { return S::add(p, q); });
      if (lane == 0) partials[b0.slot] = acc;
    } else {
#pragma unroll
      for (int k = 0; k < kPer; ++k) prod[lane + k * kWave] = pr[k];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int nrows = b0.row_end - b0.row_start;
      int L = 1;
      {
        const int avg = nrows > 0 ? nnz / nrows : 0;
        while (L < kWave && L * 4 < avg) L <<= 1;
        while (L < kWave && nrows * L * 2 <= kWave) L <<= 1;
      }
      const int groups = kWave / L;
      const int g = lane / L, l = lane % L;
      for (int base = 0; base < nrows; base += groups) {
        const int rr = base + g;        // < 64 always: a tile holds at most kWaveRows rows
        const int s = __shfl(rlo0, rr, kWave) - b0.nnz_start;
        const int e = __shfl(rhi0, rr, kWave) - b0.nnz_start;
        T acc = S::identity();
        for (int q = s + l; q < e; q += L) acc = S::add(acc, prod[q]);
        acc = group_reduce(acc, L, [](T p, T q) { return S::add(p, q); });
        if (rr < nrows && l == 0) spmv_store<SR, T>(w, b0.row_start + rr, acc, mask, mask_f32, scmp, accum);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }

    // ---- rotate: the gathers of tile i+1 land here
    GRB_HUB_PRODUCTS(b1, c1, a1, xg, xl)
    b0 = b1; rlo0 = rlo1; rhi0 = rhi1;
    b1 = b2; rlo1 = rlo2; rhi1 = rhi2;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { c1[k] = c2[k]; a1[k] = a2[k]; }
    b2 = b3;
  }
#undef GRB_HUB_STREAM
#undef GRB_HUB_GATHER
#undef GRB_HUB_PRODUCTS
#undef GRB_HUB_COLD
#undef GRB_HUB_LDS_INDEX
}

// true commutative monoids only: the column-sorted format sums a row in column-rank order, by atomics
template <int SR>
constexpr bool cband_monoid_ok() {
  if constexpr (SR == GRB_RUNTIME_SR) return false;
  else {
    constexpr int op = MonoidTraits<SemiringTraits<SR>::monoid>::op;
    return op == OP_PLUS || op == OP_TIMES || op == OP_MIN || op == OP_MAX || op == OP_LOR || op == OP_LAND;
  }
}

grb_info k_spmv(int sr, int dtype, const CsrArrays& M, SpmvPlan& plan, const void* u, const void* mask,
                int mask_f32, int scmp, int accum, void* w, const Index* other_ptr) {
  if (plan.ntiles == 0 && M.nvals > 0) return GRB_INVALID_OBJECT;   // nonzeros but no plan: never a silent no-op
  if (plan.ntiles == 0 && plan.nrows == 0) return GRB_SUCCESS;       // nothing to write
  if (M.nvals > 0 && !plan.hub_ready) {
    static const bool trace = getenv("GRB_SPMV_PREP_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    GRB_TRY(prepare_hub_packing(M, plan, other_ptr));
    if (trace) {
      (void)hipStreamSynchronize(ctx().stream);
      fprintf(stderr, "hub packing (column ranks): %8.3f ms\n",
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
  }
  return dispatch_semiring(sr, dtype, [&](auto tag, auto t) -> grb_info {
    using T = decltype(t);
    constexpr int SR = decltype(tag)::value;
    if (M.nvals == 0) {
      hipLaunchKernelGGL((spmv_empty_kernel<SR, T>), dim3(ceil_div(plan.nrows, kBlock)), dim3(kBlock), 0,
                         ctx().stream, plan.nrows, mask, mask_f32, scmp, accum, (T*)w);
      GRB_HIP_TRY(hipGetLastError());
      return GRB_SUCCESS;
    }
    const int fmt = spmv_format_setting(-1);
    if constexpr (cband_monoid_ok<SR>()) {
      if (fmt == 2 || (fmt == 1 && plan.d_order)) {
        if (!plan.cband && !plan.cband_tried && (fmt == 2 || plan.csr_launches >= spmv_reuse_threshold(-1))) {
          static const bool trace = getenv("GRB_SPMV_PREP_TRACE") != nullptr;
          const auto t0 = std::chrono::steady_clock::now();
          const grb_info pi = prepare_cband(M, plan);
          if (trace) {
            (void)hipStreamSynchronize(ctx().stream);
            fprintf(stderr, "cband prep, all of it:      %8.3f ms\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
          }
          if (pi != GRB_SUCCESS && pi != GRB_OUT_OF_MEMORY) return pi;     // no room for the second copy: CSR it is
          if (plan.cband && plan.d_ind2 && fmt == 1) {      // the CSR kernel's renamed column ids are not needed any more
            GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
            (void)hipFree(plan.d_ind2);
            plan.d_ind2 = nullptr;
          }
        }
        if (plan.cband) {
          SpmvCBand& C = *plan.cband;
          if (C.nhot > 0) {
            const Index np = plan.npacked < (Index)C.nhot ? plan.npacked : (Index)C.nhot;
            hipLaunchKernelGGL((cband_pack_kernel<T>), dim3(ceil_div(ceil_div(np, 4), kBlock)), dim3(kBlock), 0, ctx().stream, (const T*)u,
                               (const Index*)plan.d_order, np, (T*)plan.d_u2);
          }
          static const bool want_trace = getenv("GRB_SPMV_TRACE") != nullptr;
          unsigned long long* d_trace = nullptr;
          if (want_trace) {
            void* p_tr;
            GRB_TRY(scratch(10, 16 * (size_t)C.grid, &p_tr));
            d_trace = (unsigned long long*)p_tr;
          }
          if (C.iso)
            hipLaunchKernelGGL((spmv_cband_kernel<SR, T, true>), dim3(C.grid), dim3(kCbThreads), 0, ctx().stream, C.args,
                               (const T*)plan.d_u2, (const T*)u, C.nhot, mask, mask_f32, scmp, accum, (T*)w, C.d_partials, d_trace);
          else
            hipLaunchKernelGGL((spmv_cband_kernel<SR, T, false>), dim3(C.grid), dim3(kCbThreads), 0, ctx().stream, C.args,
                               (const T*)plan.d_u2, (const T*)u, C.nhot, mask, mask_f32, scmp, accum, (T*)w, C.d_partials, d_trace);
          GRB_HIP_TRY(hipGetLastError());
          if (C.nfin > 0) {
            hipLaunchKernelGGL((spmv_cband_fold_kernel<SR, T>), dim3(ceil_div(C.max_fin_rows, kWave), C.nfin), dim3(kCbFoldWaves * kWave), 0,
                               ctx().stream, C.args, (const void*)C.d_partials, mask, mask_f32, scmp, accum, (T*)w);
            GRB_HIP_TRY(hipGetLastError());
          }
          if (want_trace) {                                  // per-workgroup wall clock of the main kernel
            std::vector<unsigned long long> h(2 * (size_t)C.grid);
            GRB_HIP_TRY(hipMemcpy(h.data(), d_trace, 16 * (size_t)C.grid, hipMemcpyDeviceToHost));
            unsigned long long t0 = ~0ull, t1 = 0;
            double sum = 0, mx = 0, mn = 1e30;
            for (int g = 0; g < C.grid; ++g) {
              t0 = h[2 * g] < t0 ? h[2 * g] : t0;
              t1 = h[2 * g + 1] > t1 ? h[2 * g + 1] : t1;
              const double d = (double)(h[2 * g + 1] - h[2 * g]);
              sum += d; mx = d > mx ? d : mx; mn = d < mn ? d : mn;
            }
            fprintf(stderr, "spmv_cband_kernel workgroups (wall-clock ticks, 100 MHz): span %llu, busy min %.0f mean %.0f max %.0f\n",
                    t1 - t0, mn, sum / C.grid, mx);
            static int dumped = 0;
            if (atoi(getenv("GRB_SPMV_TRACE")) >= 2 && dumped++ == 2)
              for (int g = 0; g < C.grid; ++g)
                fprintf(stderr, "  wg %3d items %d groups %6d of which hub %6d: start %6llu ticks %6llu\n", g, C.wg_items[g],
                        C.wg_groups[g], C.wg_hub_groups[g], h[2 * g] - t0, h[2 * g + 1] - h[2 * g]);
          }
          return GRB_SUCCESS;
        }
      }
    }
    ++plan.csr_launches;
    GRB_TRY(ensure_renamed_columns(M, plan));
    const Index* ind = M.ind;
    const T* uu = (const T*)u;
    if (plan.d_ind2 || plan.bands) {
      hipLaunchKernelGGL((pack_vector_kernel<T>), dim3(ceil_div(plan.npacked, kBlock)), dim3(kBlock), 0,
                         ctx().stream, (const T*)u, plan.d_order, plan.npacked, (T*)plan.d_u2);
      ind = plan.d_ind2;
      uu = (const T*)plan.d_u2;
    }
    if (plan.bands) {
      SpmvBands& B = *plan.bands;
      hipLaunchKernelGGL((spmv_band_kernel<SR, T>), dim3(B.args.grid), dim3(kHubThreads), 0, ctx().stream, B.args, uu, mask,
                         mask_f32, scmp, accum, (T*)w, (T*)B.d_partials, (T*)B.d_t);
      GRB_HIP_TRY(hipGetLastError());
      if (B.nlong) {
        hipLaunchKernelGGL((spmv_long_finalize_kernel<SR, T>), dim3(ceil_div(B.nlong * kFinalLanes, kBlock)), dim3(kBlock),
                           0, ctx().stream, B.d_long_row, B.d_long_slot_ptr, B.nlong, (const T*)B.d_partials, mask,
                           mask_f32, scmp, accum, (T*)w);
        GRB_HIP_TRY(hipGetLastError());
      }
      return GRB_SUCCESS;
    }
    int grid = ceil_div(plan.ntiles, kHubWaves);
    if (grid > ctx().num_cu * kHubPerCu) grid = ctx().num_cu * kHubPerCu;
    hipLaunchKernelGGL((spmv_hub_kernel<SR, T>), dim3(grid), dim3(kHubThreads), 0, ctx().stream, plan.d_tiles,
                       plan.ntiles, M.ptr, ind, (const T*)M.val, uu, plan.nhot, mask, mask_f32, scmp, accum, (T*)w,
                       (T*)plan.d_partials);
    GRB_HIP_TRY(hipGetLastError());
    if (plan.nlong) {
      hipLaunchKernelGGL((spmv_long_finalize_kernel<SR, T>), dim3(ceil_div(plan.nlong * kFinalLanes, kBlock)),
                         dim3(kBlock), 0, ctx().stream, plan.d_long_row, plan.d_long_slot_ptr, plan.nlong,
                         (const T*)plan.d_partials, mask, mask_f32, scmp, accum, (T*)w);
      GRB_HIP_TRY(hipGetLastError());
    }
    return GRB_SUCCESS;
  });
}

// the column-sorted format of this orientation, if it has been prepared: what one launch streams (coded entries,
// values unless iso, group bases; the packed vector written and read; the result; the hub band's partial slices)
int k_spmv_cband_info(const SpmvPlan& plan, long long* groups, int* bands, int* items, int* hub_rows, int* iso,
                      long long* bytes_per_launch) {
  if (!plan.cband) return 0;
  const SpmvCBand& C = *plan.cband;
  *groups = C.ngroups;
  *bands = C.nbands;
  *items = C.nitems;
  *hub_rows = C.args.nhub;
  *iso = C.iso ? 1 : 0;
  const long long per_group = (C.iso ? 256 : 512) + 4;
  // coded entries (+ values) + bases; the result; the input vector once + the hot prefix's pack (order, gather,
  // store); the hub band's partial slices written and read
  *bytes_per_launch = C.ngroups * per_group + 4ll * plan.nrows + 4ll * plan.nminor + 12ll * C.nhot +
                      16ll * C.partial_elems;
  return 1;
}

grb_info k_spmv_plan_info(const CsrArrays& M, SpmvPlan& plan, const Index* other_ptr, int warm, int* bands,
                          long long* band_nnz, long long* pieces, int* nhot) {
  if (warm && M.nvals > 0 && !plan.hub_ready) GRB_TRY(prepare_hub_packing(M, plan, other_ptr));
  if (warm && M.nvals > 0 && spmv_format_setting(-1) == 0) GRB_TRY(ensure_renamed_columns(M, plan));
  *bands = plan.bands ? plan.bands->args.k : (plan.hub_ready && plan.nhot > 0 ? 1 : 0);
  *band_nnz = plan.bands ? plan.bands->band_nnz : 0;
  *pieces = plan.bands ? plan.bands->pieces : 0;
  *nhot = plan.nhot;
  return GRB_SUCCESS;
}

// ------------------------------------------------------------------------------------
// Boolean pull step with fused mask.
//   skip row            when  scmp XOR (mask[row] == 0)
//   discoverable(row)   when  some neighbour col has  (opreuse ? mask[col] != 0
//                                                              : u[col] != identity)
//   w[row] = discoverable ? 1 : 0   for EVERY row
constexpr int kSerialProbe = 8;

template <typename T, bool kOpReuse>
__device__ inline bool pull_hit(const void* mask, int mask_f32, const T* u, T identity, Index col) {
  if constexpr (kOpReuse) return mask_nonzero(mask, mask_f32, col);
  else return u[col] != identity;
}

template <typename T, bool kEarlyExit, bool kOpReuse>
__global__ __launch_bounds__(kBlock) void spmv_masked_or_kernel(
    const Index* __restrict__ ptr, const Index* __restrict__ ind, Index nrows, const T* __restrict__ u,
    T identity, const void* __restrict__ mask, int mask_f32, int scmp, const Index* __restrict__ hint,
    T* __restrict__ w) {
  const int lane = lane_id();
  const Index wave_global = (Index)blockIdx.x * kWavesPerBlock + wave_id();
  const Index nwaves = (Index)gridDim.x * kWavesPerBlock;
  for (Index base = wave_global * kWave; base < nrows; base += nwaves * kWave) {
    const Index row = base + lane;
    bool active = false, found = false;
    Index s = 0, e = 0;
    if (row < nrows) {
      active = !(mask_nonzero(mask, mask_f32, row) ? (scmp != 0) : (scmp == 0));
      // equivalently: skip when scmp XOR (mask == 0)
      if (active) { s = ptr[row]; e = ptr[row + 1]; }
    }
    // phase 0: the row's most promising neighbour from a dense side array (one coalesced 4-byte
    // read instead of an adjacency-list cache line); a hit settles the row whatever EarlyExit says,
    // because the only output is the flag
    Index p = s;
    if (active && hint) {
      const Index h = hint[row];
      if (h >= 0 && pull_hit<T, kOpReuse>(mask, mask_f32, u, identity, h)) { found = true; p = e; }
    }
    // phase 1: each lane probes up to kSerialProbe of its own neighbours
    if (active && !found) {
      Index stop = (e - s > kSerialProbe) ? s + kSerialProbe : e;
      for (; p < stop; ++p) {
        if (pull_hit<T, kOpReuse>(mask, mask_f32, u, identity, ind[p])) {
          found = true;
          if (kEarlyExit) break;
        }
      }
      if (found && kEarlyExit) p = e;
    }
    // phase 2: rows with neighbours left are finished by the whole wave, one at a time
    unsigned long long todo = __ballot(active && p < e);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const Index rs = __shfl(p, src, kWave), re = __shfl(e, src, kWave);
      bool any = false;
      for (Index q = rs; q < re; q += kWave) {
        bool h = false;
        if (q + lane < re) h = pull_hit<T, kOpReuse>(mask, mask_f32, u, identity, ind[q + lane]);
        if (__ballot(h)) { any = true; if (kEarlyExit) break; }
      }
      if (lane == src && any) found = true;
    }
    if (row < nrows) w[row] = found ? (T)1 : (T)0;
  }
}

grb_info k_spmv_masked_or(int dtype, const CsrArrays& M, const void* u, double identity, const void* mask,
                          int mask_f32, int scmp, int earlyexit, int opreuse, const Index* hint, void* w) {
  if (M.n <= 0) return GRB_SUCCESS;
  const int grid = stream_grid(M.n, kBlock);
  auto launch = [&](auto t) -> grb_info {
    using T = decltype(t);
#define GRB_PULL(EE, OR)                                                                          \
  hipLaunchKernelGGL((spmv_masked_or_kernel<T, EE, OR>), dim3(grid), dim3(kBlock), 0, ctx().stream, \
                     M.ptr, M.ind, M.n, (const T*)u, (T)identity, mask, mask_f32, scmp, hint, (T*)w)
    if (earlyexit && opreuse) GRB_PULL(true, true);
    else if (earlyexit) GRB_PULL(true, false);
    else if (opreuse) GRB_PULL(false, true);
    else GRB_PULL(false, false);
#undef GRB_PULL
    GRB_HIP_TRY(hipGetLastError());
    return GRB_SUCCESS;
  };
  if (dtype == GRB_F32) return launch(float{});
  return launch(int{});
}

}  // namespace grb
