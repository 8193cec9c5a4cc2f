// spgemm.hip -- the unmasked product C = op(A) (+.x) op(B) for f32 matrices (grb_mxm without a mask; the reference's
// cusparse_spgemm2, backend/cuda/spgemm.hpp, which always computes plus-times: here every semiring is honoured).
//
// Gustavson, row by row, in two passes over the same row bins:
//   bins      ub(i) = sum over k in row i of op(A) of |row k of op(B)| (products of the row) and da(i) = |row i of op(A)|
//             put every row into one of three lists (rows without products are in none: their count stays 0)
//               tiny16  ub <= 16 and da <= 16   a 16-lane group per row (four rows per wave)
//               tiny64  ub <= 64 and da <= 64   a wave per row
//               mid     ub <= kMidCap           a wave per row, the row's products sorted in LDS
//               wide    the rest                a wave per row and column WINDOW, dense accumulator in LDS
//   symbolic  distinct columns per row -> the row pointers (64-bit total checked against INT32_MAX first)
//   numeric   the same kernels with values: C's columns ascending, C(i,j) = add(mul(a_ik, b_kj), acc) over k ascending
// The fold is the same for every semiring, order-free monoid or not: products are folded in ascending k exactly as
// spgemm_masked_kernel folds them, so results are bit for bit those of the sequential loop, and two calls agree.
//   tiny     the row's (j, k-position) pairs, one per lane, are sorted by (j, position) across the group (bitonic, in
//            registers), and the first lane of every run of equal j folds the run in order.
//   wide     a window of kWideCols columns is a bitmap + value array in the wave's LDS.  The row's products that fall in
//            the window (each partner row cut to it by two binary searches) form one flat index space in k-major
//            order, taken 64 at a time; inside a 64-product chunk two lanes may meet the same column, so the chunk is
//            sorted as in the tiny path and each run folded onto the accumulator by its first lane.  Chunks go in
//            order, so every column sees its products in ascending k.  The window is emitted by scanning its bitmap.
//            A window starts at the smallest product column not yet emitted (the wave minimum over the partner rows
//            of their first column past the previous window), so no window is empty: a row visits at most
//            min(span / kWideCols, outputs) windows, and only rows of more than kMidCap products come here.
//   mid      the row's products (column, k-major position) written to LDS, bitonic-sorted there by the wave, runs
//            folded in order: the cost follows the products whatever the columns' spread.
// The symbolic pass skips the values.  Temporaries: the row pointers (m + 1), four row lists (4 m) and the
// result arrays; nothing is proportional to the number of products.
#include "row_bins.hpp"

namespace grb {

constexpr int kTinySmall = 16;         // lanes per row of the first bin
constexpr int kWideCols = 4096;        // columns per window of the wide kernel (16 KiB of values + 512 B of bits per wave)
constexpr int kMidCap = 1024;          // products per row of the mid bin (8 KiB of keys + 4 KiB of values per wave)

// ascending bitonic sort of (key, val) across aligned groups of L lanes; keys are distinct but for the sentinel
template <int L, typename K, typename V>
__device__ inline void spgemm_group_sort(K& key, V& val, int t) {
#pragma unroll
  for (int k = 2; k <= L; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const K ok = __shfl_xor(key, j, kWave);
      const V ov = __shfl_xor(val, j, kWave);
      const bool up = (t & k) == 0;
      const bool lower = (t & j) == 0;
      const bool take = (lower == up) ? (ok < key) : (ok > key);
      if (take) { key = ok; val = ov; }
    }
  }
}

// ub, da -> bin lists (wave-aggregated appends; the order inside a list does not matter: rows are independent)
__global__ __launch_bounds__(kBlock) void spgemm_bin_kernel(const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                            const Index* __restrict__ b_ptr, Index m, Index* __restrict__ lists,
                                                            unsigned int* __restrict__ ctr) {
  const int lane = lane_id();
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long base = (long long)blockIdx.x * kBlock + wave_id() * kWave; base < m; base += stride) {
    const Index i = (Index)(base + lane);
    int bin = -1;
    if (i < m) {
      const Index as = a_ptr[i], ae = a_ptr[i + 1];
      unsigned int ub = 0;
      for (Index e = as; e < ae; ++e) {
        const Index k = a_ind[e];
        ub += (unsigned int)(b_ptr[k + 1] - b_ptr[k]);
      }
      const Index da = ae - as;
      if (ub > 0)
        bin = (ub <= (unsigned)kTinySmall && da <= kTinySmall) ? 0 : (ub <= (unsigned)kWave && da <= kWave) ? 1 : ub <= (unsigned)kMidCap ? 2 : 3;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const unsigned long long mask = __ballot(bin == b);
      if (!mask) continue;
      const int leader = __ffsll((long long)mask) - 1;
      unsigned int at = 0;
      if (lane == leader) at = atomicAdd(&ctr[b], (unsigned int)__popcll(mask));
      at = (unsigned int)__shfl((int)at, leader, kWave);
      if (bin == b) lists[(size_t)b * m + at + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
  }
}

// rows of at most L products and L entries: an L-lane group each
template <int SR, typename T, int L, bool kNum>
__global__ __launch_bounds__(kBlock) void spgemm_tiny_kernel(const Index* __restrict__ rows, Index nrows,
                                                             const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                             const T* __restrict__ a_val, const Index* __restrict__ b_ptr,
                                                             const Index* __restrict__ b_ind, const T* __restrict__ b_val,
                                                             unsigned int* __restrict__ counts, const Index* __restrict__ c_ptr,
                                                             Index* __restrict__ c_ind, T* __restrict__ c_val) {
  typedef Semiring<SR, T> S;
  constexpr int kGroups = kWave / L;                     // rows per wave
  __shared__ unsigned long long s_key[kNum ? kBlock : 1];
  __shared__ T s_prod[kNum ? kBlock : 1];
  const int lane = lane_id(), t = lane & (L - 1);
  const unsigned long long gmask = L == kWave ? ~0ull : (((1ull << (L % kWave)) - 1ull) << (lane & ~(L - 1)));
  const long long step = (long long)gridDim.x * kWavesPerBlock * kGroups;
  for (long long w0 = ((long long)blockIdx.x * kWavesPerBlock + wave_id()) * kGroups; w0 < nrows; w0 += step) {
    const long long g = w0 + lane / L;
    const bool live = g < nrows;
    const Index r = live ? rows[g] : 0;
    Index as = 0, da = 0;
    if (live) { as = a_ptr[r]; da = a_ptr[r + 1] - as; }
    Index bs = 0, len = 0;
    T a = T(0);
    if (t < da) {
      const Index k = a_ind[as + t];
      bs = b_ptr[k];
      len = b_ptr[k + 1] - bs;
      if constexpr (kNum) a = a_val[as + t];
    }
    Index incl = len;
#pragma unroll
    for (int o = 1; o < L; o <<= 1) {
      const Index y = __shfl_up(incl, o, L);
      if (t >= o) incl += y;
    }
    const Index total = __shfl(incl, L - 1, L);
    const Index excl = incl - len;                       // = total for the lanes past the row's entries
    // product t of the row: owner = the last entry whose first product is <= t
    const bool valid = t < total;
    int o = 0;
#pragma unroll
    for (int s = L / 2; s > 0; s >>= 1) {
      const Index e = __shfl(excl, o + s, L);
      if (e <= t) o += s;
    }
    const Index o_bs = __shfl(bs, o, L), o_ex = __shfl(excl, o, L);
    const T o_a = __shfl(a, o, L);
    unsigned long long key = ~0ull;
    T prod = T(0);
    if (valid) {
      const Index q = o_bs + t - o_ex;
      key = ((unsigned long long)(unsigned int)b_ind[q] << 6) | (unsigned long long)t;
      if constexpr (kNum) prod = S::mul(o_a, b_val[q]);
    }
    spgemm_group_sort<L>(key, prod, t);
    const unsigned long long prev = __shfl_up(key, 1, L);
    const bool head = key != ~0ull && (t == 0 || (prev >> 6) != (key >> 6));
    const unsigned long long hm = __ballot(head) & gmask;
    if constexpr (!kNum) {
      if (live && t == 0) counts[r] = (unsigned int)__popcll(hm);
    } else {
      s_key[threadIdx.x] = key;
      s_prod[threadIdx.x] = prod;
      wave_lds_sync();
      if (head) {
        const int g0 = threadIdx.x - t;
        T acc = S::identity();
        for (int u = t; u < L && (s_key[g0 + u] >> 6) == (key >> 6); ++u) acc = S::add(s_prod[g0 + u], acc);
        const Index pos = c_ptr[r] + __popcll(hm & ((1ull << lane) - 1ull));
        c_ind[pos] = (Index)(key >> 6);
        c_val[pos] = acc;
      }
      wave_lds_sync();
    }
  }
}

// every other row: a wave per row, the row's product columns in windows of kWideCols (see the top of the file)
template <int SR, typename T, bool kNum>
__global__ __launch_bounds__(kWave) void spgemm_wide_kernel(const Index* __restrict__ rows, Index nrows,
                                                            const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                            const T* __restrict__ a_val, const Index* __restrict__ b_ptr,
                                                            const Index* __restrict__ b_ind, const T* __restrict__ b_val,
                                                            unsigned int* __restrict__ counts, const Index* __restrict__ c_ptr,
                                                            Index* __restrict__ c_ind, T* __restrict__ c_val) {
  typedef Semiring<SR, T> S;
  constexpr int kWords = kWideCols / 32;
  __shared__ T s_acc[kNum ? kWideCols : 1];
  __shared__ unsigned int s_bits[kWords];
  __shared__ Index s_off[kWave], s_lo[kWave];
  __shared__ T s_a[kNum ? kWave : 1];
  __shared__ unsigned int s_key[kNum ? kWave : 1];
  __shared__ T s_prod[kNum ? kWave : 1];
  const int lane = lane_id();
  for (Index g = blockIdx.x; g < nrows; g += gridDim.x) {
    const Index r = rows[g];
    const Index as = a_ptr[r], ae = a_ptr[r + 1];
    if constexpr (!kNum) {
      if (ae - as == 1) {                                // one partner row: its columns are the row's
        if (lane == 0) { const Index k = a_ind[as]; counts[r] = (unsigned int)(b_ptr[k + 1] - b_ptr[k]); }
        continue;
      }
    }
    // the span of the row's product columns
    unsigned int jmin = 0xffffffffu, jend = 0u;
    for (Index e = as + lane; e < ae; e += kWave) {
      const Index k = a_ind[e];
      const Index bs = b_ptr[k], be = b_ptr[k + 1];
      if (be > bs) {
        const unsigned int lo = (unsigned int)b_ind[bs], hi = (unsigned int)b_ind[be - 1] + 1u;
        jmin = lo < jmin ? lo : jmin;
        jend = hi > jend ? hi : jend;
      }
    }
    jmin = wave_min_u32(jmin);
    jend = wave_max_u32(jend);
    Index out = 0;
    if constexpr (kNum) out = c_ptr[r];
    unsigned int cnt = 0;
    for (long long w0 = jmin; w0 < (long long)jend;) {
      unsigned int wnext = 0xffffffffu;                  // the smallest product column past this window
      const Index wlo = (Index)w0;
      const Index whi = (Index)((long long)jend < w0 + kWideCols ? (long long)jend : w0 + kWideCols);
      for (int i = lane; i < kWords; i += kWave) s_bits[i] = 0u;
      wave_lds_sync();
      for (Index c0 = as; c0 < ae; c0 += kWave) {
        const Index e = c0 + lane;
        Index lo = 0, len = 0;
        unsigned int nxt = 0xffffffffu;
        T a = T(0);
        if (e < ae) {
          const Index k = a_ind[e];
          const Index bs = b_ptr[k], be = b_ptr[k + 1];
          if (be > bs) {
            lo = b_ind[bs] >= wlo ? bs : index_lower_bound(b_ind, bs, be, wlo);
            const Index hi = b_ind[be - 1] < whi ? be : index_lower_bound(b_ind, lo, be, whi);
            len = hi - lo;                                 // <= kWideCols: a row's columns are distinct
            if (hi < be) nxt = (unsigned int)b_ind[hi];
          }
          if constexpr (kNum) a = a_val[e];
        }
        wnext = min(wnext, wave_min_u32(nxt));
        const unsigned int incl = wave_incl_scan_u32((unsigned int)len);
        const Index total = (Index)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        if (total == 0) continue;
        s_off[lane] = (Index)incl - len;
        s_lo[lane] = lo;
        if constexpr (kNum) s_a[lane] = a;
        wave_lds_sync();
        for (Index x0 = 0; x0 < total; x0 += kWave) {
          const Index x = x0 + lane;
          const bool valid = x < total;
          unsigned int key = 0xffffffffu;
          T prod = T(0);
          if (valid) {
            int o = 0;
#pragma unroll
            for (int s = kWave / 2; s > 0; s >>= 1)
              if (s_off[o + s] <= x) o += s;
            const Index q = s_lo[o] + (x - s_off[o]);
            const unsigned int jr = (unsigned int)(b_ind[q] - wlo);
            if constexpr (kNum) {
              prod = S::mul(s_a[o], b_val[q]);
              key = (jr << 6) | (unsigned int)lane;
            } else {
              atomicOr(&s_bits[jr >> 5], 1u << (jr & 31u));
            }
          }
          if constexpr (kNum) {
            spgemm_group_sort<kWave>(key, prod, lane);
            s_key[lane] = key;
            s_prod[lane] = prod;
            wave_lds_sync();
            const unsigned int prev = lane > 0 ? s_key[lane - 1] : 0xffffffffu;
            const bool head = key != 0xffffffffu && (lane == 0 || (prev >> 6) != (key >> 6));
            if (head) {
              const unsigned int jr = key >> 6, bit = 1u << (jr & 31u);
              T acc = (s_bits[jr >> 5] & bit) ? s_acc[jr] : S::identity();
              for (int u = lane; u < kWave && (s_key[u] >> 6) == jr; ++u) acc = S::add(s_prod[u], acc);
              s_acc[jr] = acc;
              atomicOr(&s_bits[jr >> 5], bit);
            }
          }
          wave_lds_sync();
        }
      }
      // the window's columns, ascending
      for (int wb = 0; wb < kWords; wb += kWave) {
        unsigned int word = wb + lane < kWords ? s_bits[wb + lane] : 0u;
        const unsigned int pc = (unsigned int)__popc(word);
        const unsigned int incl = wave_incl_scan_u32(pc);
        const unsigned int tot = (unsigned int)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        if constexpr (kNum) {
          Index pos = out + (Index)(incl - pc);
          while (word) {
            const int b = __ffs(word) - 1;
            word &= word - 1u;
            const int col = (wb + lane) * 32 + b;
            c_ind[pos] = wlo + col;
            c_val[pos] = s_acc[col];
            ++pos;
          }
        }
        out += (Index)tot;
        cnt += tot;
      }
      wave_lds_sync();
      w0 = wnext;                                        // (> the window: the loop ends when no partner has more)
    }
    if constexpr (!kNum)
      if (lane == 0) counts[r] = cnt;
  }
}

// rows of more than 64 and at most kMidCap products: the row's products as (column << 10 | k-major position) keys in the
// wave's LDS, bitonic-sorted there, each run of one column folded in order by its first element's lane
template <int SR, typename T, bool kNum>
__global__ __launch_bounds__(kWave) void spgemm_mid_kernel(const Index* __restrict__ rows, Index nrows,
                                                           const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                           const T* __restrict__ a_val, const Index* __restrict__ b_ptr,
                                                           const Index* __restrict__ b_ind, const T* __restrict__ b_val,
                                                           unsigned int* __restrict__ counts, const Index* __restrict__ c_ptr,
                                                           Index* __restrict__ c_ind, T* __restrict__ c_val) {
  typedef Semiring<SR, T> S;
  static_assert(kMidCap <= 1024, "the position takes the key's low 10 bits");
  __shared__ unsigned long long s_key[kMidCap];
  __shared__ T s_val[kNum ? kMidCap : 1];
  __shared__ Index s_off[kWave], s_lo[kWave];
  __shared__ T s_a[kNum ? kWave : 1];
  const int lane = lane_id();
  for (Index g = blockIdx.x; g < nrows; g += gridDim.x) {
    const Index r = rows[g];
    const Index as = a_ptr[r], ae = a_ptr[r + 1];
    // ---- expand: product x of the row (k-major) at position np + x
    Index np = 0;
    for (Index c0 = as; c0 < ae; c0 += kWave) {
      const Index e = c0 + lane;
      Index lo = 0, len = 0;
      T a = T(0);
      if (e < ae) {
        const Index k = a_ind[e];
        lo = b_ptr[k];
        len = b_ptr[k + 1] - lo;
        if constexpr (kNum) a = a_val[e];
      }
      const unsigned int incl = wave_incl_scan_u32((unsigned int)len);
      const Index total = (Index)__builtin_amdgcn_readlane((int)incl, kWave - 1);   // np + total <= kMidCap (the bin)
      if (total == 0) continue;
      s_off[lane] = (Index)incl - len;
      s_lo[lane] = lo;
      if constexpr (kNum) s_a[lane] = a;
      wave_lds_sync();
      for (Index x = lane; x < total; x += kWave) {
        int o = 0;
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1)
          if (s_off[o + s] <= x) o += s;
        const Index q = s_lo[o] + (x - s_off[o]);
        const Index at = np + x;
        s_key[at] = ((unsigned long long)(unsigned int)b_ind[q] << 10) | (unsigned long long)at;
        if constexpr (kNum) s_val[at] = S::mul(s_a[o], b_val[q]);
      }
      np += total;
      wave_lds_sync();
    }
    // ---- sort the np keys (padded to a power of two with the largest key)
    int P = kWave;
    while (P < np) P <<= 1;
    for (int i = np + lane; i < P; i += kWave) s_key[i] = ~0ull;
    wave_lds_sync();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = lane; i < P; i += kWave) {
          const int p = i ^ j;
          if (p > i) {
            const unsigned long long ki = s_key[i], kp = s_key[p];
            if ((ki > kp) == ((i & k) == 0)) {
              s_key[i] = kp;
              s_key[p] = ki;
              if constexpr (kNum) { const T v = s_val[i]; s_val[i] = s_val[p]; s_val[p] = v; }
            }
          }
        }
        wave_lds_sync();
      }
    }
    // ---- runs of one column: count them, fold each in order
    Index out = 0;
    if constexpr (kNum) out = c_ptr[r];
    unsigned int cnt = 0;
    for (Index i0 = 0; i0 < np; i0 += kWave) {
      const Index i = i0 + lane;
      const bool valid = i < np;
      const unsigned long long key = valid ? s_key[i] : ~0ull;
      const bool head = valid && (i == 0 || (s_key[i - 1] >> 10) != (key >> 10));
      const unsigned long long hm = __ballot(head);
      if constexpr (kNum) {
        if (head) {
          T acc = S::identity();
          for (Index u = i; u < np && (s_key[u] >> 10) == (key >> 10); ++u) acc = S::add(s_val[u], acc);
          const Index pos = out + (Index)cnt + __popcll(hm & ((1ull << lane) - 1ull));
          c_ind[pos] = (Index)(key >> 10);
          c_val[pos] = acc;
        }
      }
      cnt += (unsigned int)__popcll(hm);
    }
    if constexpr (!kNum)
      if (lane == 0) counts[r] = cnt;
    wave_lds_sync();
  }
}

grb_info spgemm_unmasked(grb_matrix C, int op, grb_matrix A, grb_matrix B, bool tran_a, bool tran_b) {
  if (C == A || C == B) return GRB_NOT_IMPLEMENTED;
  if (A->dtype != GRB_F32 || B->dtype != GRB_F32 || C->dtype != GRB_F32) return GRB_NOT_IMPLEMENTED;   // the reference's scope
  const CsrArrays& Aa = tran_a ? A->csc : A->csr;        // rows of op(A)
  const CsrArrays& Bb = tran_b ? B->csc : B->csr;        // rows of op(B)
  if (!Aa.ptr || !Bb.ptr) return GRB_INVALID_OBJECT;
  const Index m = tran_a ? A->ncols : A->nrows, kin = tran_a ? A->nrows : A->ncols;
  const Index kb = tran_b ? B->ncols : B->nrows, n = tran_b ? B->nrows : B->ncols;
  if (kin != kb || C->nrows != m || C->ncols != n) return GRB_DIMENSION_MISMATCH;
  if (Aa.n != m || Bb.n != kb) return GRB_INVALID_OBJECT;   // (a CSR-only matrix's "CSC" of another shape)
  hipStream_t s = ctx().stream;
  // ---- bins
  EwmBuf d_ptr, d_work;
  const size_t scan_bytes = device_scan_u32_scratch((long long)m + 1);
  GRB_TRY(ewm_alloc(&d_ptr, 4 * ((size_t)m + 1)));
  GRB_TRY(ewm_alloc(&d_work, 64 + 4 * 4 * (size_t)m + scan_bytes));
  unsigned int* counts = (unsigned int*)d_ptr.p;
  unsigned int* ctr = (unsigned int*)d_work.p;            // [4] bin sizes, then the 64-bit total (8-byte aligned)
  unsigned long long* d_total = (unsigned long long*)(ctr + 4);
  Index* lists = (Index*)((char*)d_work.p + 64);          // [4][m] rows of each bin
  unsigned int* scan_totals = (unsigned int*)(lists + 4 * (size_t)m);
  GRB_HIP_TRY(hipMemsetAsync(counts, 0, 4 * ((size_t)m + 1), s));
  GRB_HIP_TRY(hipMemsetAsync(ctr, 0, 64, s));
  if (m > 0 && Aa.nvals > 0 && Bb.nvals > 0) {
    hipLaunchKernelGGL(spgemm_bin_kernel, dim3(stream_grid(m, kBlock)), dim3(kBlock), 0, s, Aa.ptr, Aa.ind, Bb.ptr, m, lists, ctr);
    GRB_HIP_TRY(hipGetLastError());
  }
  unsigned int nbin[4] = {0, 0, 0, 0};
  GRB_HIP_TRY(hipMemcpyAsync(nbin, ctr, 16, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  const Index* l16 = lists;
  const Index* l64 = lists + m;
  const Index* lmid = lists + 2 * (size_t)m;
  const Index* lwide = lists + 3 * (size_t)m;
  const int tiny16_grid = capped_grid(nbin[0], kBlock / kTinySmall), tiny64_grid = capped_grid(nbin[1], kWavesPerBlock);
  const int mid_grid = capped_grid(nbin[2], 1), wide_grid = capped_grid(nbin[3], 1);   // (a wave per row: one-wave workgroups)
  const float* av = (const float*)Aa.val;
  const float* bv = (const float*)Bb.val;
  // ---- symbolic (semiring-free: the plus-times instantiation without values)
  if (nbin[0]) hipLaunchKernelGGL((spgemm_tiny_kernel<GRB_PLUS_MULTIPLIES, float, kTinySmall, false>), dim3(tiny16_grid), dim3(kBlock), 0, s,
                                  l16, (Index)nbin[0], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, counts, nullptr, nullptr, nullptr);
  if (nbin[1]) hipLaunchKernelGGL((spgemm_tiny_kernel<GRB_PLUS_MULTIPLIES, float, kWave, false>), dim3(tiny64_grid), dim3(kBlock), 0, s,
                                  l64, (Index)nbin[1], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, counts, nullptr, nullptr, nullptr);
  if (nbin[2]) hipLaunchKernelGGL((spgemm_mid_kernel<GRB_PLUS_MULTIPLIES, float, false>), dim3(mid_grid), dim3(kWave), 0, s,
                                  lmid, (Index)nbin[2], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, counts, nullptr, nullptr, nullptr);
  if (nbin[3]) hipLaunchKernelGGL((spgemm_wide_kernel<GRB_PLUS_MULTIPLIES, float, false>), dim3(wide_grid), dim3(kWave), 0, s,
                                  lwide, (Index)nbin[3], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, counts, nullptr, nullptr, nullptr);
  GRB_HIP_TRY(hipGetLastError());
  unsigned long long total = 0;
  if (m > 0) {
    hipLaunchKernelGGL(count_total_kernel, dim3(stream_grid(m, kBlock * 8)), dim3(kBlock), 0, s, counts, m, nullptr, 0, d_total);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  if (total > (unsigned long long)INT32_MAX) return GRB_OUT_OF_MEMORY;   // grb_index is 32 bits; C keeps what it held
  const Index nnz = (Index)total;
  GRB_TRY(device_exclusive_scan_u32_in(counts, (long long)m + 1, scan_totals));   // counts -> row pointers
  std::vector<Index> h_ptr((size_t)m + 1);
  GRB_HIP_TRY(hipMemcpy(h_ptr.data(), counts, 4 * ((size_t)m + 1), hipMemcpyDeviceToHost));
  EwmBuf d_ind, d_val;
  GRB_TRY(ewm_alloc(&d_ind, 4 * (size_t)(nnz > 0 ? nnz : 1)));
  GRB_TRY(ewm_alloc(&d_val, 4 * (size_t)(nnz > 0 ? nnz : 1)));
  // ---- numeric
  if (nnz > 0) {
    GRB_TRY(dispatch_semiring(op, GRB_F32, [&](auto tag, auto t) -> grb_info {
      using T = decltype(t);
      constexpr int SR = decltype(tag)::value;
      if constexpr (!std::is_same<T, float>::value) {
        return GRB_NOT_IMPLEMENTED;
      } else {
        const Index* cp = (const Index*)counts;
        Index* ci = (Index*)d_ind.p;
        T* cv = (T*)d_val.p;
        if (nbin[0]) hipLaunchKernelGGL((spgemm_tiny_kernel<SR, T, kTinySmall, true>), dim3(tiny16_grid), dim3(kBlock), 0, s, l16,
                                        (Index)nbin[0], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, nullptr, cp, ci, cv);
        if (nbin[1]) hipLaunchKernelGGL((spgemm_tiny_kernel<SR, T, kWave, true>), dim3(tiny64_grid), dim3(kBlock), 0, s, l64,
                                        (Index)nbin[1], Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, nullptr, cp, ci, cv);
        if (nbin[2]) hipLaunchKernelGGL((spgemm_mid_kernel<SR, T, true>), dim3(mid_grid), dim3(kWave), 0, s, lmid, (Index)nbin[2],
                                        Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, nullptr, cp, ci, cv);
        if (nbin[3]) hipLaunchKernelGGL((spgemm_wide_kernel<SR, T, true>), dim3(wide_grid), dim3(kWave), 0, s, lwide, (Index)nbin[3],
                                        Aa.ptr, Aa.ind, av, Bb.ptr, Bb.ind, bv, nullptr, cp, ci, cv);
        GRB_HIP_TRY(hipGetLastError());
        return GRB_SUCCESS;
      }
    }));
  }
  GRB_HIP_TRY(hipStreamSynchronize(s));
  // ---- C is replaced as the masked product replaces it: CSR only, owned arrays, plan built at first use
  matrix_release_device(C);
  C->owned = true;
  C->nvals = nnz;
  C->csr.ptr = (Index*)d_ptr.release();
  C->csr.ind = (Index*)d_ind.release();
  C->csr.val = d_val.release();
  C->csr.n = m;
  C->csr.nvals = nnz;
  C->h_csr_ptr.swap(h_ptr);
  C->h_csr_ind.clear(); C->h_csr_val.clear();
  C->h_csc_ptr.clear(); C->h_csc_ind.clear(); C->h_csc_val.clear();
  C->nonneg_values = -1; C->mean_value = -1.0; C->small_int_values = -1;
  C->plan_csr_pending = true;
  C->built = true;
  return GRB_SUCCESS;
}

}  // namespace grb
