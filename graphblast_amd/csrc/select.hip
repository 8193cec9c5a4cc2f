// select.hip -- GraphBLAS's select (GrB_select with the predefined index-unary operators; the reference has no such
// operation): grb_matrix_select, grb_vector_select.  The contract is the comment in include/grb_hip.h.
//
// One orientation X (pointers, indices, values) is a flat list of nnz entries, and select is a stream compaction of that
// list: entry-balanced, whatever the rows look like.
//   tiles     the entries [0, nnz) in tiles of kSelTile = 2048: a workgroup per tile, a wave per 512 consecutive entries, a
//             lane per entry in each of eight steps of 64 -- every load and every store is a run of consecutive words.
//   count     the predicate of every entry; a step's ballot is its 64 flags, the population counts of a tile's 32 ballots
//             are the tile's kept entries: one count per tile.
//   scan      device_exclusive_scan_u32 over the tile counts: a tile's offset, and the total = the result's nvals.
//   write     the predicate again; an entry's place is its tile's offset + the kept entries of the waves and steps
//             before it + the set flags below its lane in its step's ballot.  No atomics, no scan instruction: the order
//             of the entries is the order of the list.  The same launch writes the new pointers: row r's is the rank of
//             the old ptr[r] in the compacted list, taken from the ballots of the wave whose entries (w0, w1] hold it --
//             empty rows and rows that lose everything included.
//   rows      a positional predicate needs an entry's row.  A wave finds the row of its first entry by one search of ptr
//             (64 probes per round: four rounds for 2^22 rows), notes in LDS which rows begin at which of its entries
//             (lanes over the rows that follow, until one begins past the wave's last entry) and takes a running maximum
//             over the steps: a hub row that began many tiles earlier is the search's answer, and a run of thousands of
//             empty rows is 64 rows per round of that loop.  Value predicates read no index and no pointer in the count.
// X's other orientation, the transposed read and the vector forms are the same kernels: with the roles of i and j
// exchanged, TRIL k is TRIU -k, DIAG k is DIAG -k, ROWLE is COLLE and so on (sel_swap), and a vector is the one row
// j = 0 of that exchanged form (no pointers; a dense vector's index is the position).
#include "common.hpp"

#include <cmath>

namespace grb {

constexpr int kSelSteps = 8;                             // entries per lane
constexpr int kSelWaveTile = kWave * kSelSteps;          // consecutive entries of one wave
constexpr int kSelTile = kSelWaveTile * kWavesPerBlock;  // ... of one workgroup: one count, one offset

// inclusive running maximum over the wave's lanes (wave_incl_scan_u32 with v_max; every lane must be active)
__device__ __forceinline__ unsigned wave_incl_scan_max_u32(unsigned v) {
  auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
  unsigned t = mx(mx(v, __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false)),
                  mx(__builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0u, v, 0x113, 0xf, 0xf, false)));
  t = mx(t, __builtin_amdgcn_update_dpp(0u, t, 0x114, 0xf, 0xe, false));
  t = mx(t, __builtin_amdgcn_update_dpp(0u, t, 0x118, 0xf, 0xc, false));
  t = mx(t, __builtin_amdgcn_update_dpp(0u, t, 0x142, 0xa, 0xf, false));
  t = mx(t, __builtin_amdgcn_update_dpp(0u, t, 0x143, 0xc, 0xf, false));
  return t;
}

// the largest r with ptr[r] <= x, for 0 <= x < ptr[nrows]: the row of entry x.  The whole wave probes, 64 places a round.
__device__ inline Index sel_find_row(const Index* __restrict__ ptr, Index nrows, long long x, int lane) {
  long long lo = 0, hi = nrows;                          // ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const long long step = (hi - lo + kWave - 1) / kWave;
    const long long q = lo + (lane + 1) * step;
    const bool le = q < hi && (long long)ptr[q] <= x;
    lo += __popcll(__ballot(le)) * step;                 // (ptr ascends: the probes that pass are the first ones)
    hi = lo + step < hi ? lo + step : hi;
  }
  return (Index)lo;
}

// i, j: row and column in the orientation the kernel reads; 64-bit, so i + k cannot wrap
template <int OP>
__device__ __forceinline__ bool sel_pos(long long i, long long j, long long k) {
  if constexpr (OP == GRB_SEL_TRIL) return j <= i + k;
  if constexpr (OP == GRB_SEL_TRIU) return j >= i + k;
  if constexpr (OP == GRB_SEL_DIAG) return j == i + k;
  if constexpr (OP == GRB_SEL_OFFDIAG) return j != i + k;
  if constexpr (OP == GRB_SEL_ROWLE) return i <= k;
  if constexpr (OP == GRB_SEL_ROWGT) return i > k;
  if constexpr (OP == GRB_SEL_COLLE) return j <= k;
  return j > k;                                          // GRB_SEL_COLGT
}
template <int OP, typename T>
__device__ __forceinline__ bool sel_val(T a, T k) {
  if constexpr (OP == GRB_SEL_VALUEEQ) return a == k;
  if constexpr (OP == GRB_SEL_VALUENE) return a != k;
  if constexpr (OP == GRB_SEL_VALUELT) return a < k;
  if constexpr (OP == GRB_SEL_VALUELE) return a <= k;
  if constexpr (OP == GRB_SEL_VALUEGT) return a > k;
  return a >= k;                                         // GRB_SEL_VALUEGE
}

// kWrite false: tiles[t] = the kept entries of tile t.  kWrite true: tiles[t] is tile t's offset; the kept entries and,
// with pointers, new_ptr are written.  ptr == nullptr: every entry is in row 0 (the vector forms); ind == nullptr: an
// entry's index is its position (a dense vector).  T: the values' type for a value predicate, unsigned for a positional
// one, which never looks at them.  One workgroup per tile.
template <int OP, typename T, bool kWrite>
__global__ __launch_bounds__(kBlock) void sel_kernel(const Index* __restrict__ ptr, Index nrows, const Index* __restrict__ ind,
                                                     const unsigned int* __restrict__ val, long long nnz, long long kpos, T kval,
                                                     unsigned int* __restrict__ tiles, Index* __restrict__ new_ptr,
                                                     Index* __restrict__ out_ind, unsigned int* __restrict__ out_val) {
  constexpr bool kPos = OP < GRB_SEL_VALUEEQ;
  __shared__ unsigned int s_head[kPos ? kSelTile : 1];   // the row that begins at an entry of the tile (0: none does)
  __shared__ int s_wave[kWavesPerBlock];
  const int lane = lane_id(), wid = wave_id();
  const long long w0 = (long long)blockIdx.x * kSelTile + (long long)wid * kSelWaveTile;
  const long long w1 = w0 + kSelWaveTile < nnz ? w0 + kSelWaveTile : nnz;   // the wave's entries: [w0, w1)
  const bool live = w0 < nnz;                            // wave-uniform
  const bool rows = ptr != nullptr && live;
  Index rw = 0;                                          // the row of entry w0
  if (rows && (kPos || kWrite)) rw = sel_find_row(ptr, nrows, w0, lane);
  if constexpr (kPos) {
    if (rows) {
      unsigned int* head = s_head + wid * kSelWaveTile;
#pragma unroll
      for (int k = 0; k < kSelSteps; ++k) head[k * kWave + lane] = 0u;
      // other lanes of this wave write row numbers over these zeros: order the two stores across the wave's lanes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // the rows after rw that begin inside the wave and are not empty (an empty row shares its start with the next one)
      for (long long r = (long long)rw + 1 + lane;; r += kWave) {
        bool ok = false;
        if (r < nrows) {
          const Index p = ptr[r];
          ok = p < w1;
          if (ok && ptr[r + 1] > p) head[(int)(p - w0)] = (unsigned int)r;
        }
        if (__ballot(ok) != ~0ull) break;
      }
    }
    __syncthreads();
  }
  // ---- the flags: eight ballots
  Index c[kSelSteps];
  unsigned int v[kSelSteps];
#pragma unroll
  for (int k = 0; k < kSelSteps; ++k) {
    const long long e = w0 + k * kWave + lane;
    c[k] = 0;
    v[k] = 0u;
    if (e < w1) {
      if constexpr (kPos || kWrite) c[k] = ind ? ind[e] : (Index)e;
      if constexpr (!kPos || kWrite) v[k] = val[e];
    }
  }
  unsigned long long m[kSelSteps];
  unsigned int carry = (unsigned int)rw;
  int kept = 0;
#pragma unroll
  for (int k = 0; k < kSelSteps; ++k) {
    const bool in = w0 + k * kWave + lane < w1;
    bool pass;
    if constexpr (kPos) {
      unsigned int row = 0u;
      if (ptr) {                                         // (uniform over the launch)
        const unsigned int h = rows ? s_head[wid * kSelWaveTile + k * kWave + lane] : 0u;
        row = wave_incl_scan_max_u32(h);
        row = row > carry ? row : carry;
        carry = (unsigned int)__builtin_amdgcn_readlane((int)row, kWave - 1);
      }
      pass = in && sel_pos<OP>((long long)row, (long long)c[k], kpos);
    } else {
      T a;
      memcpy(&a, &v[k], 4);
      pass = in && sel_val<OP, T>(a, kval);
    }
    m[k] = __ballot(pass);
    kept += __popcll(m[k]);
  }
  if (lane == 0) s_wave[wid] = kept;
  __syncthreads();
  if constexpr (!kWrite) {
    if (threadIdx.x == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) sum += s_wave[w];
      tiles[blockIdx.x] = (unsigned int)sum;
    }
  } else {
    unsigned int base = tiles[blockIdx.x];               // the wave's first place in the result
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) base += w < wid ? (unsigned int)s_wave[w] : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned int at = base;
#pragma unroll
    for (int k = 0; k < kSelSteps; ++k) {
      if ((m[k] >> lane) & 1ull) {
        const unsigned int pos = at + (unsigned int)__popcll(m[k] & below);
        out_ind[pos] = c[k];
        out_val[pos] = v[k];
      }
      at += (unsigned int)__popcll(m[k]);
    }
    if (!rows) return;
    // the new pointers of the rows whose old one lies in (w0, w1]: base + the kept entries of the wave before it.  Those
    // that are 0 (the rows up to the row of entry 0) fall to the first wave.
    if (w0 == 0)
      for (long long r = lane; r <= (long long)rw; r += kWave) new_ptr[r] = 0;
    for (long long r = (long long)rw + 1 + lane;; r += kWave) {
      bool ok = false;
      if (r <= nrows) {
        const Index p = ptr[r];
        ok = p <= w1;
        if (ok) {
          const int d = (int)(p - w0);                   // in (0, kSelWaveTile]
          int rank = 0;
#pragma unroll
          for (int k = 0; k < kSelSteps; ++k) {
            const int b = d - k * kWave;                 // the flags of step k below the old pointer
            const unsigned long long sel = b >= kWave ? ~0ull : b <= 0 ? 0ull : (1ull << b) - 1ull;
            rank += __popcll(m[k] & sel);
          }
          new_ptr[r] = (Index)(base + (unsigned int)rank);
        }
      }
      if (__ballot(ok) != ~0ull) break;
    }
  }
}

namespace {

// the same predicate with the roles of i and j exchanged: what the other orientation (and a vector, the row j = 0) is asked
void sel_swap(int* op, long long* k) {
  switch (*op) {
    case GRB_SEL_TRIL: *op = GRB_SEL_TRIU; *k = -*k; break;   // j <= i + k  <=>  i >= j - k
    case GRB_SEL_TRIU: *op = GRB_SEL_TRIL; *k = -*k; break;
    case GRB_SEL_DIAG: case GRB_SEL_OFFDIAG: *k = -*k; break;
    case GRB_SEL_ROWLE: *op = GRB_SEL_COLLE; break;
    case GRB_SEL_ROWGT: *op = GRB_SEL_COLGT; break;
    case GRB_SEL_COLLE: *op = GRB_SEL_ROWLE; break;
    case GRB_SEL_COLGT: *op = GRB_SEL_ROWGT; break;
    default: break;                                      // a value predicate has no roles
  }
}

// the operator and the thunk, checked (grb_hip.h); *kpos: the positional thunk, clamped to +-2^62, far outside j - i
grb_info sel_check(int op, int dtype, double thunk, long long* kpos) {
  if (op < 0 || op >= GRB_N_SELECT_OPS) return GRB_INVALID_VALUE;
  *kpos = 0;
  if (op < GRB_SEL_VALUEEQ) {
    if (!std::isfinite(thunk) || thunk != std::floor(thunk)) return GRB_INVALID_VALUE;   // NaN, an infinity, a fraction
    const double lim = 4611686018427387904.0;            // 2^62
    *kpos = thunk >= lim ? (1ll << 62) : thunk <= -lim ? -(1ll << 62) : (long long)thunk;
  } else if (dtype == GRB_I32) {
    if (!(thunk >= -2147483648.0 && thunk <= 2147483647.0) || thunk != (double)(int)thunk) return GRB_INVALID_VALUE;
  }
  return GRB_SUCCESS;
}

template <typename F>
grb_info sel_dispatch(int op, int dtype, F&& f) {
#define GRB_CASE(OP)                                                         \
  case OP:                                                                   \
    if constexpr ((OP) < GRB_SEL_VALUEEQ) return f(IntTag<OP>{}, 0u);        \
    else if (dtype == GRB_F32) return f(IntTag<OP>{}, float{});              \
    else return f(IntTag<OP>{}, int{});
  switch (op) {
    GRB_CASE(GRB_SEL_TRIL) GRB_CASE(GRB_SEL_TRIU) GRB_CASE(GRB_SEL_DIAG) GRB_CASE(GRB_SEL_OFFDIAG)
    GRB_CASE(GRB_SEL_ROWLE) GRB_CASE(GRB_SEL_ROWGT) GRB_CASE(GRB_SEL_COLLE) GRB_CASE(GRB_SEL_COLGT)
    GRB_CASE(GRB_SEL_VALUEEQ) GRB_CASE(GRB_SEL_VALUENE) GRB_CASE(GRB_SEL_VALUELT) GRB_CASE(GRB_SEL_VALUELE)
    GRB_CASE(GRB_SEL_VALUEGT) GRB_CASE(GRB_SEL_VALUEGE)
    default: return GRB_INVALID_VALUE;
  }
#undef GRB_CASE
}

// The three steps over one list of nnz > 0 entries.  ptr nullable (then new_ptr is not written), ind nullable.  The result's
// arrays are allocated here, for exactly the kept entries (*kept).  The write is left in flight: the caller synchronises
// the stream before it uses the result, and keeps the tile offsets (*tiles) until then.
grb_info sel_compact(const Index* ptr, Index nrows, const Index* ind, const void* val, Index nnz, int dtype, int op, long long kpos,
                     double thunk, Index* new_ptr, EwmBuf* tiles, EwmBuf* o_ind, EwmBuf* o_val, Index* kept) {
  hipStream_t s = ctx().stream;
  const int ntiles = (int)(((long long)nnz + kSelTile - 1) / kSelTile);
  GRB_TRY(ewm_alloc(tiles, 4 * ((size_t)ntiles + 1) + device_scan_u32_scratch((long long)ntiles + 1)));
  unsigned int* d_tiles = (unsigned int*)tiles->p;
  unsigned int* d_scan = d_tiles + ntiles + 1;
  GRB_HIP_TRY(hipMemsetAsync(d_tiles + ntiles, 0, 4, s));
  auto launch = [&](auto write) -> grb_info {
    return sel_dispatch(op, dtype, [&](auto tag, auto t) -> grb_info {
      typedef decltype(t) T;
      T kv;
      if constexpr (std::is_same<T, float>::value) kv = (float)thunk;
      else if constexpr (std::is_same<T, int>::value) kv = (int)thunk;
      else kv = 0u;
      hipLaunchKernelGGL((sel_kernel<decltype(tag)::value, T, decltype(write)::value != 0>), dim3(ntiles), dim3(kBlock), 0, s, ptr, nrows,
                         ind, (const unsigned int*)val, (long long)nnz, kpos, kv, d_tiles, new_ptr, (Index*)o_ind->p,
                         (unsigned int*)o_val->p);
      GRB_HIP_TRY(hipGetLastError());
      return GRB_SUCCESS;
    });
  };
  GRB_TRY(launch(IntTag<0>{}));
  GRB_TRY(device_exclusive_scan_u32_in(d_tiles, (long long)ntiles + 1, d_scan));
  unsigned int total = 0;
  GRB_HIP_TRY(hipMemcpy(&total, d_tiles + ntiles, 4, hipMemcpyDeviceToHost));
  *kept = (Index)total;
  GRB_TRY(ewm_alloc(o_ind, 4 * (size_t)(total > 0 ? total : 1)));
  GRB_TRY(ewm_alloc(o_val, 4 * (size_t)(total > 0 ? total : 1)));
  return launch(IntTag<1>{});
}

// one orientation: out = the entries of X that pass
grb_info select_side(const CsrArrays& X, Index nrows, int dtype, int op, long long kpos, double thunk, Side* out) {
  EwmBuf tiles;                                          // (freed after the synchronisation below)
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)nrows + 1)));
  if (X.nvals > 0) {
    GRB_TRY(sel_compact(X.ptr, nrows, X.ind, X.val, X.nvals, dtype, op, kpos, thunk, (Index*)out->ptr.p, &tiles, &out->ind, &out->val,
                        &out->nnz));
  } else {
    GRB_HIP_TRY(hipMemsetAsync(out->ptr.p, 0, 4 * ((size_t)nrows + 1), ctx().stream));
    GRB_TRY(ewm_alloc(&out->ind, 4));
    GRB_TRY(ewm_alloc(&out->val, 4));
  }
  out->h_ptr.resize((size_t)nrows + 1);
  GRB_HIP_TRY(hipMemcpyAsync(out->h_ptr.data(), out->ptr.p, 4 * ((size_t)nrows + 1), hipMemcpyDeviceToHost, ctx().stream));
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return GRB_SUCCESS;
}

}  // namespace

grb_info select_matrix(grb_matrix C, grb_matrix A, int op, double thunk, bool tran) {
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  const Index m = tran ? A->ncols : A->nrows, n = tran ? A->nrows : A->ncols;   // op(A) is m x n
  if (C->nrows != m || C->ncols != n) return GRB_DIMENSION_MISMATCH;
  long long kpos = 0;
  GRB_TRY(sel_check(op, A->dtype, thunk, &kpos));
  if ((tran && !has_csc(A)) || !A->csr.ptr) return GRB_INVALID_OBJECT;
  const CsrArrays& Xr = tran ? A->csc : A->csr;          // rows of op(A)
  const CsrArrays& Xc = tran ? A->csr : A->csc;          // its columns
  const bool both = C->format != 1 && (tran || has_csc(A));
  Side r, c;
  GRB_TRY(select_side(Xr, m, A->dtype, op, kpos, thunk, &r));
  if (both) {
    int op_c = op;
    long long k_c = kpos;
    sel_swap(&op_c, &k_c);
    GRB_TRY(select_side(Xc, n, A->dtype, op_c, k_c, thunk, &c));
  }
  return attach(C, &r, both ? &c : nullptr);             // (A may be C: both sides have synchronised)
}

grb_info select_vector(grb_vector w, grb_vector u, int op, double thunk) {
  if (u->vec_type != GRB_SPARSE && u->vec_type != GRB_DENSE) return GRB_UNINITIALIZED_OBJECT;
  if (w->dtype != u->dtype) return GRB_DOMAIN_MISMATCH;
  if (w->nsize != u->nsize) return GRB_DIMENSION_MISMATCH;
  long long kpos = 0;
  GRB_TRY(sel_check(op, u->dtype, thunk, &kpos));
  sel_swap(&op, &kpos);                                  // a vector is the row j = 0 of the exchanged form
  hipStream_t s = ctx().stream;
  const bool sparse = u->vec_type == GRB_SPARSE;
  const Index cnt = sparse ? u->s_nvals : u->nsize;
  EwmBuf tiles, o_ind, o_val;                            // (w may be u: its storage is written last)
  Index kept = 0;
  if (cnt > 0)
    GRB_TRY(sel_compact(nullptr, 1, sparse ? u->s_ind : nullptr, sparse ? u->s_val : u->d_val, cnt, u->dtype, op, kpos, thunk, nullptr,
                        &tiles, &o_ind, &o_val, &kept));
  // everything that can fail is behind us
  GRB_TRY(grb_vector_set_storage(w, GRB_SPARSE));
  if (kept > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(w->s_ind, o_ind.p, 4 * (size_t)kept, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemcpyAsync(w->s_val, o_val.p, 4 * (size_t)kept, hipMemcpyDeviceToDevice, s));
  }
  GRB_HIP_TRY(hipStreamSynchronize(s));
  w->s_nvals = kept;
  w->nvals = kept;
  return GRB_SUCCESS;
}

}  // namespace grb

using namespace grb;

// select: the contract is the comment in include/grb_hip.h
grb_info grb_matrix_select(grb_matrix C, grb_matrix mask, grb_accum accum, int select_op, double thunk, grb_matrix A,
                           grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  if (!C || !A) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built || (mask && !mask->built)) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return select_matrix(C, A, select_op, thunk, desc && desc->desc[GRB_INP0] == GRB_TRAN);
}

grb_info grb_vector_select(grb_vector w, grb_vector mask, grb_accum accum, int select_op, double thunk, grb_vector u,
                           grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  (void)desc;
  if (!w || !u) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return select_vector(w, u, select_op, thunk);
}
