// bc.hip -- betweenness centrality on the device: grb_bc, batched Brandes.  The contract is the comment in
// include/grb_hip.h; the reference has no such driver (graphblas/algorithm/), the definition is LAGraph's.
//
// The sources are taken in batches of up to kBcBatch = 64: lane s of a wave is source s of the batch, and everything a
// vertex knows per source is one source-minor row of 64 values.  Structure only (no value array of A is ever read).
//   depth[v][s]   v's depth from source s, -1 where s does not reach v                       (n x 64 int)
//   sigma[v][s]   the shortest s -> v paths; after the backward pass has been at v: (1 + delta_s(v)) / sigma_s(v), the
//                 one value v's parents gather, so that the backward pass divides once per vertex and not per edge
//                                                                                             (n x 64 double)
//   list / off    the vertices that ANY source of the batch has at depth d, for every d: list[off[d] .. off[d + 1])
//   acc[v]        the sum of delta_s(v) over every source so far, s = v left out             (n double)
// sweep     level d: a workgroup per vertex of list d - 1, its out-neighbours (CSR) over the workgroup's waves; lane s
//           labels a neighbour that s has not reached; the first wave to label a vertex at level d (an integer atomicMax
//           on mark[w]) appends it to list d.  The lists come out in no fixed order; nothing below depends on it.
// forward   level d, right behind the sweep's level: a workgroup per vertex w of list d walks w's in-neighbours (CSC) in
//           stored order; lane s adds sigma[v][s] where depth[v][s] == d - 1 and depth[w][s] == d.  Wave k takes the
//           neighbours at positions 4 k .. 4 k + 3 of every 16 (16 k .. 16 k + 15 of every 64 in a row of more than
//           kBcLong entries); the four partial rows are added in wave order in LDS.
// backward  level d = L .. 1: the same shape over v's out-neighbours, gathering sigma[w][s] (by then (1 + delta) / sigma)
//           where depth[w][s] == d + 1; delta = sigma[v][s] * sum; sigma[v][s] becomes (1 + delta) / sigma[v][s]; the 64
//           deltas are added by a butterfly and acc[v] takes the sum: one workgroup per (vertex, level), levels one
//           launch after the other, so acc has one writer at a time.  Level 0 is the sources themselves: left out.
// Both passes are gathers in stored order with a fixed association and there is no floating-point atomic anywhere: the
// same inputs give the same bits.  Nothing is allocated inside the loops.  The host reads the list offsets once every
// kBcChunk levels of the sweep (launching a level past the last one costs two empty launches), and nothing else; the
// backward levels are launched back to back with grids of their lists' sizes.
#include "graph_common.hpp"

namespace grb {

constexpr int kBcBatch = kWave;                          // sources of one batch: a lane each
constexpr int kBcUnroll = 4;                             // neighbour rows a wave keeps in flight: 16 a workgroup step
constexpr int kBcLong = 256;                             // a row longer than this (a hub: one workgroup has all of it) keeps
constexpr int kBcLongUnroll = 16;                        // ... this many rows in flight per wave, 64 a workgroup step
constexpr int kBcGrid = 2048;                            // workgroups of a level's launch; a longer list is walked grid-stride
constexpr int kBcChunk = 8;                              // levels of the sweep between two host reads
typedef unsigned long long u64;

__device__ __forceinline__ size_t bc_row(Index v) { return (size_t)v * kBcBatch + lane_id(); }
__device__ __forceinline__ int bc_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// info[0]: the tail of the lists, info[1]: vertices reached (all batches)
__global__ __launch_bounds__(kBcBatch) void bc_init_kernel(const Index* __restrict__ src, int nb, Index n, int* __restrict__ depth,
                                                           double* __restrict__ sigma, int* __restrict__ mark,
                                                           Index* __restrict__ list, u64* __restrict__ off, u64* __restrict__ info) {
  const int lane = threadIdx.x;
  if (lane < nb) {
    const Index v = src[lane];
    if ((unsigned)v < (unsigned)n) {                     // (checked on the host already)
      depth[bc_row(v)] = 0;
      sigma[bc_row(v)] = 1.0;
      if (atomicMax(&mark[v], 0) < 0) list[atomicAdd(&info[0], 1ull)] = v;
    }
  }
  __syncthreads();
  if (lane == 0) {
    off[0] = 0ull;
    off[1] = atomicAdd(&info[0], 0ull);
    atomicAdd(&info[1], (u64)nb);
  }
}

// the sweep's walk over one row, U neighbours a wave per step
template <int U>
__device__ __forceinline__ void bc_sweep_row(const Index* __restrict__ ind, Index pb, Index pe, Index n, int d, bool active,
                                             int* __restrict__ depth, int* __restrict__ mark, Index* __restrict__ list,
                                             u64* __restrict__ info) {
  const int wid = bc_wave(), lane = lane_id();
  for (Index x0 = pb + wid * U; x0 < pe; x0 += U * kWavesPerBlock) {
    Index w[U];
    int dw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u] = x0 + u < pe ? ind[x0 + u] : -1;
      if ((unsigned)w[u] >= (unsigned)n) w[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) dw[u] = w[u] >= 0 ? depth[bc_row(w[u])] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool fresh = active && w[u] >= 0 && dw[u] < 0;
      if (fresh) depth[bc_row(w[u])] = d;                // (another wave may store the same d into the same word)
      if (__ballot(fresh) != 0ull && lane == 0 && atomicMax(&mark[w[u]], d) < d) list[atomicAdd(&info[0], 1ull)] = w[u];
    }
  }
}

// level d of the sweep: list d - 1 = [off[d - 1], off[d]) labels its out-neighbours and makes list d behind info[0]
__global__ __launch_bounds__(kBlock) void bc_sweep_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index n, int d,
                                                          int* __restrict__ depth, int* __restrict__ mark, Index* __restrict__ list,
                                                          const u64* __restrict__ off, u64* __restrict__ info) {
  const u64 lo = off[d - 1], hi = off[d];
  for (u64 i = lo + blockIdx.x; i < hi; i += gridDim.x) {
    const Index v = list[i];
    const bool active = depth[bc_row(v)] == d - 1;
    const Index pb = ptr[v], pe = ptr[v + 1];
    if (pe - pb > kBcLong) bc_sweep_row<kBcLongUnroll>(ind, pb, pe, n, d, active, depth, mark, list, info);
    else bc_sweep_row<kBcUnroll>(ind, pb, pe, n, d, active, depth, mark, list, info);
  }
}

// a wave's share of a gather, U neighbours a wave per step: the sum over its neighbours x of val[x][s] where
// depth[x][s] == want and `mine`
template <int U>
__device__ __forceinline__ double bc_gather_row(const Index* __restrict__ ind, Index pb, Index pe, Index n, const int* __restrict__ depth,
                                                const double* __restrict__ val, int want, bool mine) {
  const int wid = bc_wave();
  double sum = 0.0;
  for (Index x0 = pb + wid * U; x0 < pe; x0 += U * kWavesPerBlock) {
    Index w[U];
    int dw[U];
    double t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u] = x0 + u < pe ? ind[x0 + u] : -1;
      if ((unsigned)w[u] >= (unsigned)n) w[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) dw[u] = w[u] >= 0 ? depth[bc_row(w[u])] : -2;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool hit = mine && dw[u] == want;
      t[u] = 0.0;
      if (__ballot(hit) != 0ull) {                       // the 512-byte row only where some source needs it
        const double s = val[bc_row(w[u])];
        t[u] = hit ? s : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) sum += t[u];
  }
  return sum;
}

// The gather both passes share: the sum over the neighbours ind[pb .. pe), in every lane of wave 0 (the other waves
// return their own partial).  part: kWavesPerBlock x 64 doubles.
__device__ __forceinline__ double bc_gather(const Index* __restrict__ ind, Index pb, Index pe, Index n, const int* __restrict__ depth,
                                            const double* __restrict__ val, int want, bool mine, double* part) {
  const int wid = bc_wave(), lane = lane_id();
  double sum = pe - pb > kBcLong ? bc_gather_row<kBcLongUnroll>(ind, pb, pe, n, depth, val, want, mine)
                                 : bc_gather_row<kBcUnroll>(ind, pb, pe, n, depth, val, want, mine);
  __syncthreads();                                       // the partials of the vertex before this one have been read
  part[wid * kWave + lane] = sum;
  __syncthreads();
  if (wid == 0) {
    sum = part[lane];
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) sum += part[k * kWave + lane];
  }
  return sum;
}

// level d of the forward pass: list d = [off[d], info[0]) (the sweep's level d is over); off[d + 1] = info[0]
__global__ __launch_bounds__(kBlock) void bc_forward_kernel(const Index* __restrict__ iptr, const Index* __restrict__ iind, Index n, int d,
                                                            const int* __restrict__ depth, double* __restrict__ sigma,
                                                            const Index* __restrict__ list, u64* __restrict__ off, u64* __restrict__ info) {
  __shared__ double part[kBlock];
  const int wid = bc_wave();
  const u64 lo = off[d], hi = info[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) off[d + 1] = hi;
  u64 reached = 0;
  for (u64 i = lo + blockIdx.x; i < hi; i += gridDim.x) {
    const Index w = list[i];
    const bool mine = depth[bc_row(w)] == d;
    const double s = bc_gather(iind, iptr[w], iptr[w + 1], n, depth, sigma, d - 1, mine, part);
    if (wid == 0) {
      if (mine) sigma[bc_row(w)] = s;
      reached += (u64)__popcll(__ballot(mine));
    }
  }
  if (threadIdx.x == 0 && reached != 0) atomicAdd(&info[1], reached);
}

// level d of the backward pass: list d = [lo, hi)
__global__ __launch_bounds__(kBlock) void bc_backward_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index n, int d,
                                                             const int* __restrict__ depth, double* __restrict__ sigma,
                                                             const Index* __restrict__ list, u64 lo, u64 hi, double* __restrict__ acc) {
  __shared__ double part[kBlock];
  const int wid = bc_wave(), lane = lane_id();
  for (u64 i = lo + blockIdx.x; i < hi; i += gridDim.x) {
    const Index v = list[i];
    const bool mine = depth[bc_row(v)] == d;
    const double g = bc_gather(ind, ptr[v], ptr[v + 1], n, depth, sigma, d + 1, mine, part);
    if (wid == 0) {
      double delta = 0.0;
      if (mine) {
        const double sg = sigma[bc_row(v)];
        delta = sg * g;
        sigma[bc_row(v)] = (1.0 + delta) / sg;
      }
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) delta += __shfl_xor(delta, o, kWave);
      if (lane == 0) acc[v] += delta;
    }
  }
}

__global__ __launch_bounds__(kBlock) void bc_round_kernel(const double* __restrict__ acc, Index n, float* __restrict__ out) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v < n) out[v] = (float)acc[v];
}

namespace {

inline int bc_grid(u64 items, Index n) {
  u64 g = items < (u64)kBcGrid ? items : (u64)kBcGrid;
  if (g > (u64)n) g = (u64)n;
  return (int)(g > 0 ? g : 1);
}

grb_info bc_run(grb_vector bc, grb_matrix A, const std::vector<Index>& src, grb_bc_result* res) {
  GRB_TRY(ctx_init());
  hipStream_t s = ctx().stream;
  const Index n = A->nrows;
  const int ns = (int)src.size();
  grb_bc_result out = {};
  out.sources = ns;
  EventPair ev;
  GRB_TRY(ev.create());
  // ---- everything the call needs, up front
  const size_t rows = (size_t)n * kBcBatch, noff = (size_t)n + kBcChunk + 8;
  EwmBuf b_depth, b_sigma, b_list, b_small;
  GRB_TRY(ewm_alloc(&b_depth, 4 * rows));
  GRB_TRY(ewm_alloc(&b_sigma, 8 * rows));
  GRB_TRY(ewm_alloc(&b_list, sizeof(Index) * rows));
  // acc [n] double, off [noff] u64, info [2] u64, mark [n] int, the sources [ns]
  GRB_TRY(ewm_alloc(&b_small, 8 * ((size_t)n + noff + 2) + 4 * ((size_t)n + (size_t)ns) + 64));
  int* d_depth = (int*)b_depth.p;
  double* d_sigma = (double*)b_sigma.p;
  Index* d_list = (Index*)b_list.p;
  double* d_acc = (double*)b_small.p;
  u64* d_off = (u64*)(d_acc + n);
  u64* d_info = d_off + noff;
  int* d_mark = (int*)(d_info + 2);
  Index* d_src = (Index*)(d_mark + n);
  GRB_TRY(dense_out_prepare(bc, n));                     // bc is as it was until the result is there (bc_round_kernel writes it)
  GRB_HIP_TRY(hipMemsetAsync(d_acc, 0, 8 * (size_t)n, s));
  GRB_HIP_TRY(hipMemsetAsync(d_info, 0, 16, s));
  GRB_HIP_TRY(hipMemcpyAsync(d_src, src.data(), sizeof(Index) * (size_t)ns, hipMemcpyHostToDevice, s));
  const Index *optr = A->csr.ptr, *oind = A->csr.ind;
  const Index *iptr = A->csc_alias ? A->csr.ptr : A->csc.ptr, *iind = A->csc_alias ? A->csr.ind : A->csc.ind;
  std::vector<u64> h_off;
  GRB_HIP_TRY(hipEventRecord(ev.a, s));
  for (int b0 = 0; b0 < ns; b0 += kBcBatch) {
    const int nb = ns - b0 < kBcBatch ? ns - b0 : kBcBatch;
    GRB_HIP_TRY(hipMemsetAsync(d_depth, 0xff, 4 * rows, s));
    GRB_HIP_TRY(hipMemsetAsync(d_mark, 0xff, 4 * (size_t)n, s));
    GRB_HIP_TRY(hipMemsetAsync(d_info, 0, 8, s));
    hipLaunchKernelGGL(bc_init_kernel, dim3(1), dim3(kBcBatch), 0, s, d_src + b0, nb, n, d_depth, d_sigma, d_mark, d_list, d_off, d_info);
    GRB_HIP_TRY(hipGetLastError());
    // ---- the sweep with the forward pass behind every level; last = the largest depth any source reaches
    h_off.assign(2, 0ull);
    int last = -1;
    for (int d0 = 1; last < 0; d0 += kBcChunk) {
      for (int d = d0; d < d0 + kBcChunk; ++d) {
        hipLaunchKernelGGL(bc_sweep_kernel, dim3(bc_grid(kBcGrid, n)), dim3(kBlock), 0, s, optr, oind, n, d, d_depth, d_mark, d_list, d_off,
                           d_info);
        hipLaunchKernelGGL(bc_forward_kernel, dim3(bc_grid(kBcGrid, n)), dim3(kBlock), 0, s, iptr, iind, n, d, d_depth, d_sigma, d_list,
                           d_off, d_info);
      }
      GRB_HIP_TRY(hipGetLastError());
      h_off.resize((size_t)d0 + kBcChunk + 1);
      GRB_HIP_TRY(hipMemcpyAsync(h_off.data() + d0, d_off + d0, 8 * ((size_t)kBcChunk + 1), hipMemcpyDeviceToHost, s));
      GRB_HIP_TRY(hipStreamSynchronize(s));
      for (int d = d0; d < d0 + kBcChunk && last < 0; ++d)
        if (h_off[d + 1] == h_off[d]) last = d - 1;      // list d is empty
      if (last < 0 && d0 + kBcChunk > n) return GRB_PANIC;   // (no depth reaches n)
    }
    if (last + 1 > out.levels) out.levels = last + 1;
    // ---- the backward pass
    for (int d = last; d >= 1; --d)
      hipLaunchKernelGGL(bc_backward_kernel, dim3(bc_grid(h_off[d + 1] - h_off[d], n)), dim3(kBlock), 0, s, optr, oind, n, d, d_depth,
                         d_sigma, d_list, h_off[d], h_off[d + 1], d_acc);
    GRB_HIP_TRY(hipGetLastError());
    ++out.batches;
  }
  GRB_HIP_TRY(hipEventRecord(ev.b, s));
  u64 h_info[2] = {0, 0};
  GRB_HIP_TRY(hipMemcpyAsync(h_info, d_info, 16, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // every kernel has run: nothing can fail from here on
  hipLaunchKernelGGL(bc_round_kernel, dim3(ceil_div(n, kBlock)), dim3(kBlock), 0, s, d_acc, n, (float*)bc->d_val);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipStreamSynchronize(s));
  bc->vec_type = GRB_DENSE;
  bc->d_nnz = n;
  GRB_HIP_TRY(hipEventElapsedTime(&out.loop_ms, ev.a, ev.b));
  out.reached = (int64_t)h_info[1];
  if (res) *res = out;
  return GRB_SUCCESS;
}

}  // namespace
}  // namespace grb

using namespace grb;

// betweenness centrality: the contract is the comment in include/grb_hip.h
grb_info grb_bc(grb_vector bc, grb_matrix A, const grb_index* sources, int ns, grb_descriptor desc, grb_bc_result* result) { GRB_API_ENTER();
  (void)desc;
  if (!bc || !A || !A->built) return GRB_UNINITIALIZED_OBJECT;
  if (A->nrows != A->ncols || bc->nsize != A->nrows) return GRB_DIMENSION_MISMATCH;
  const Index n = A->nrows;
  if (sources && ns < 1) return GRB_INVALID_VALUE;
  std::vector<Index> src;
  if (sources) {
    for (int i = 0; i < ns; ++i)
      if (sources[i] < 0 || sources[i] >= n) return GRB_INVALID_INDEX;
    src.assign(sources, sources + ns);
  } else {
    src.resize((size_t)n);
    for (Index v = 0; v < n; ++v) src[v] = v;
  }
  if (bc->dtype != GRB_F32 || (A->dtype != GRB_F32 && A->dtype != GRB_I32)) return GRB_NOT_IMPLEMENTED;
  if (!A->csr.ptr || (!A->csc_alias && !A->csc.ptr)) return GRB_INVALID_OBJECT;   // a product result: no CSC of its own
  if (n == 0) {
    if (result) *result = grb_bc_result{};
    return GRB_SUCCESS;
  }
  return bc_run(bc, A, src, result);
}
