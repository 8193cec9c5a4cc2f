// assign_matrix.hip -- the four matrix assign forms (operations.hpp:441-551: C(I, J) = A, C(I, j) = u, C(i, J) = u,
// C(I, J) = val; the reference declares them, prints "assign matrix variant not implemented yet" and returns
// GrB_NOT_IMPLEMENTED): grb_matrix_assign, grb_matrix_assign_col, grb_matrix_assign_row, grb_matrix_assign_scalar.
// The contract is the comment in include/grb_hip.h.
//
// One orientation of the new C is the row-by-row merge of the old C with T, the source placed at its targets:
//   lists     I and J are validated and inverted as extract.hip does (list_check / list_invert): the scanned histogram
//             of a list says whether an index is in the region (a count of 1), finds a repeated index (a count above 1:
//             GRB_INVALID_INDEX before anything else runs), gives its place in the list, and -- a scan of 0 / 1 flags
//             being a rank -- the ascending form of J that the constant form merges with.
//   T         a (begin, end) pair per row of C (begin < 0: the row is not in I), a column array and a value array.
//               matrix, J non-decreasing  the pairs are A's row pointers looked up through the inverse of I, the columns
//                                         J[A's columns] (A's own under a null J), the values A's: nothing is sorted
//               matrix, any other J       (I[i] << 32 | J[j], value bits) pairs through the radix sort of build.hip over
//                                         the significant bits; the pairs by binary search in the sorted keys
//               row / column              the same pairs from u's stored entries (all of a dense u), at most size(u)
//               constant                  never materialised: every selected row is the one ascending copy of J (no
//                                         column array at all under a null J) with the constant
//   bins      rows not in I, and rows whose T side is empty under an accum, keep what they hold whatever the mask says:
//             they are counted by their pointers and copied entry by entry (one balanced pass over the old C's entries,
//             an entry finding its row by binary search).  The others by merged length |old C row| + |T row|
//             (the shared pipeline of row_bins.hpp):
//               short  len <= 2 * kAShort   a 16-lane group per row (four rows per wave)
//               wave   len <= kASeg         a wave per row
//               hub    the rest             segments of kASeg merged positions, a wave each, cut at merge-path splits
//   merge     the windowed two-list merge of ewise_matrix.hip (ranks by binary search in LDS, equal columns owned by the
//             old C's element), then the rule of the contract per merged position: in both -> accum(c, t) or t; in T
//             only -> t; in C only -> kept outside J or under an accum, deleted otherwise.  With a mask the position is
//             probed in the mask row (binary search): where the mask does not pass, the old C's entry (or absence) stays.
//             Kept flags are balloted into slots.  A symbolic pass counts, the 64-bit total is checked against INT32_MAX,
//             a numeric pass writes.  No atomics on values.
// C's CSC is the same routine over the other orientations with I and J exchanged.
#include "row_bins.hpp"

namespace grb {

constexpr int kAShort = 16;             // lanes per row of the short bin (rows of at most 2 * kAShort merged positions)
constexpr int kASeg = 2048;             // the longest merged row of the wave bin; merged positions per segment of a hub row
constexpr unsigned int kANone = 0xffffffffu;   // no column: above every column index

// T of one orientation, as the kernels read it
struct AmT {
  const Index* beg;                     // [rows of C] first entry of the row's T side; < 0: the row is not in the region
  const Index* end;
  const Index* ind;                     // columns; nullptr: entry p is column p (the constant form under a null J)
  const unsigned int* val;              // value bits; nullptr: cbits everywhere (the constant form)
  unsigned int cbits;
  const Index* cptr;                    // the inverse of the column list: c is in the region when cptr[c + 1] > cptr[c];
};                                      // nullptr: every column is

__device__ inline unsigned int am_tcol(const AmT& t, Index p) { return (unsigned int)(t.ind ? t.ind[p] : p); }
template <typename T> __device__ inline T am_from(unsigned int b);
template <> __device__ inline float am_from<float>(unsigned int b) { return __uint_as_float(b); }
template <> __device__ inline int am_from<int>(unsigned int b) { return (int)b; }
__device__ inline unsigned int am_bits(float x) { return __float_as_uint(x); }
__device__ inline unsigned int am_bits(int x) { return (unsigned int)x; }

// a row that keeps what it holds: not in I, or nothing to merge under an accum
__device__ inline bool am_is_copy(const AmT& t, Index r, int accum) {
  const Index b = t.beg[r];
  return b < 0 || (accum >= 0 && t.end[r] == b);
}
// a row's merged length for the bins; the copied rows are in none
struct AmRowLen {
  const Index* a_ptr;
  AmT t;
  int accum;
  __device__ long long operator()(long long r) const {
    if (am_is_copy(t, (Index)r, accum)) return 0;
    return (long long)(a_ptr[r + 1] - a_ptr[r]) + (t.end[r] - t.beg[r]);
  }
};

// ---- lists
__global__ __launch_bounds__(kBlock) void am_dup_kernel(const Index* __restrict__ jptr, Index dim, unsigned int* __restrict__ flag) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < dim; c += stride)
    if (jptr[c + 1] - jptr[c] > 1) *flag = 1u;
}
// the ascending form of a list without repeats: the scanned 0 / 1 histogram is the rank
__global__ __launch_bounds__(kBlock) void am_selcols_kernel(const Index* __restrict__ jptr, Index dim, Index* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < dim; c += stride)
    if (jptr[c + 1] > jptr[c]) out[jptr[c]] = (Index)c;
}

// ---- T
// row r of C -> its place i in the row list (rptr == nullptr: r itself) -> x_ptr[i], x_ptr[i + 1]; x_ptr == nullptr: 0, len
__global__ __launch_bounds__(kBlock) void am_rowrange_kernel(Index m, const Index* __restrict__ rptr, const Index* __restrict__ rpos,
                                                             const Index* __restrict__ x_ptr, Index len, Index* __restrict__ beg,
                                                             Index* __restrict__ end) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < m; r += stride) {
    Index i = (Index)r;
    if (rptr) {
      const Index p = rptr[r];
      i = rptr[r + 1] > p ? (rpos ? rpos[p] : p) : -1;
    }
    beg[r] = i < 0 ? -1 : x_ptr ? x_ptr[i] : 0;
    end[r] = i < 0 ? -1 : x_ptr ? x_ptr[i + 1] : len;
  }
}
__global__ __launch_bounds__(kBlock) void am_mapcols_kernel(const Index* __restrict__ x_ind, Index nnz, const Index* __restrict__ list,
                                                            Index* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) out[p] = list[x_ind[p]];
}
// source entry p of row i (found by binary search) -> (rl[i] << 32 | cl[column], value bits); null lists: the index itself
__global__ __launch_bounds__(kBlock) void am_keys_kernel(const Index* __restrict__ x_ptr, const Index* __restrict__ x_ind,
                                                         const unsigned int* __restrict__ x_val, Index nrows, Index nnz,
                                                         const Index* __restrict__ rl, const Index* __restrict__ cl,
                                                         unsigned long long* __restrict__ keys, unsigned int* __restrict__ pay) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) {
    Index lo = 0, hi = nrows;                          // the row: the last i with x_ptr[i] <= p
    while (hi - lo > 1) {
      const Index mid = lo + ((hi - lo) >> 1);
      if (x_ptr[mid] <= (Index)p) lo = mid; else hi = mid;
    }
    const Index c = x_ind[p];
    keys[p] = ((unsigned long long)(unsigned int)(rl ? rl[lo] : lo) << 32) | (unsigned int)(cl ? cl[c] : c);
    pay[p] = x_val[p];
  }
}
// stored entry e of u (element k = u_ind[e], or e of a dense u) -> target list[k] (k under a null list) paired with `fixed`
__global__ __launch_bounds__(kBlock) void am_vec_keys_kernel(const Index* __restrict__ u_ind, const unsigned int* __restrict__ u_val,
                                                             Index nu, const Index* __restrict__ list, Index fixed, int list_major,
                                                             unsigned long long* __restrict__ keys, unsigned int* __restrict__ pay) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < nu; e += stride) {
    const Index k = u_ind ? u_ind[e] : (Index)e;
    const unsigned int x = (unsigned int)(list ? list[k] : k), f = (unsigned int)fixed;
    keys[e] = list_major ? ((unsigned long long)x << 32) | f : ((unsigned long long)f << 32) | x;
    pay[e] = u_val[e];
  }
}
// sorted keys -> the rows' (begin, end) by binary search; rptr: the inverse of the row list (nullptr: every row is in it)
__global__ __launch_bounds__(kBlock) void am_keyrange_kernel(Index m, const unsigned long long* __restrict__ keys, Index n,
                                                             const Index* __restrict__ rptr, Index* __restrict__ beg,
                                                             Index* __restrict__ end) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < m; r += stride) {
    Index b[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const unsigned long long key = (unsigned long long)(r + x) << 32;
      Index lo = 0, hi = n;
      while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      b[x] = lo;
    }
    const bool in = !rptr || rptr[r + 1] > rptr[r];
    beg[r] = in ? b[0] : -1;
    end[r] = in ? b[1] : -1;
  }
}
__global__ __launch_bounds__(kBlock) void am_unpack_kernel(const unsigned long long* __restrict__ keys, Index n, Index* __restrict__ ind) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) ind[p] = (Index)(unsigned int)keys[p];
}

// ---- bins.  tot[0 .. 3] (row_bins.hpp): short rows, wave rows, hub segments, entries of the copied rows.  The copied rows'
// counts are their lengths, written here; row_bin_kernel then fills lists that hold exactly what was counted here.
__global__ __launch_bounds__(kBlock) void am_len_kernel(AmRowLen len_of, Index m, unsigned int* __restrict__ counts,
                                                        unsigned long long* __restrict__ tot) {
  RowLenSums sums;
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < m; r += stride) {
    if (am_is_copy(len_of.t, (Index)r, len_of.accum)) {
      const Index la = len_of.a_ptr[r + 1] - len_of.a_ptr[r];
      counts[r] = (unsigned int)la;
      sums.n_own += (unsigned long long)la;
      continue;
    }
    row_len_add<2 * kAShort, kASeg>(sums, len_of(r));
  }
  row_len_totals(sums, tot);
}

// ---- the merge.  One kernel for every bin: groups of G lanes (kAShort or kWave), an item each -- a whole row (seg_k ==
// nullptr) or one segment of a hub row.  kNum = false: counts only.  List A is the old C's row, list B the row's T side.
// A merged position's kind: 0 in the old C only, 1 in both, 2 in T only.
template <typename T, int G, bool kNum>
__global__ __launch_bounds__(kBlock) void am_merge_kernel(const Index* __restrict__ items, const Index* __restrict__ seg_k, Index nitems,
                                                          const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                          const unsigned int* __restrict__ a_val, AmT tt,
                                                          const Index* __restrict__ m_ptr, const Index* __restrict__ m_ind,
                                                          const void* __restrict__ m_val, int mask_f32, int scmp, int accum,
                                                          unsigned int* __restrict__ counts, unsigned int* __restrict__ seg_cnt,
                                                          const Index* __restrict__ c_ptr, const unsigned int* __restrict__ seg_off,
                                                          Index* __restrict__ c_ind, unsigned int* __restrict__ c_val) {
  __shared__ unsigned int s_a[kBlock], s_b[kBlock], s_col[kBlock];
  __shared__ unsigned char s_kind[kBlock];
  __shared__ unsigned int s_z[kNum ? kBlock : 1], s_c[kNum ? kBlock : 1];
  const int lane = lane_id(), t = lane & (G - 1);
  const int g0 = threadIdx.x - t;                      // the group's first slot in the LDS arrays
  const unsigned long long gmask = G == kWave ? ~0ull : (((1ull << (G % kWave)) - 1ull) << (lane & ~(G - 1)));
  const unsigned long long below = (1ull << lane) - 1ull;
  constexpr int kGroups = kBlock / G;
  const long long step = (long long)gridDim.x * kGroups;
  for (long long it = (long long)blockIdx.x * kGroups + threadIdx.x / G; it < nitems; it += step) {
    const Index r = items[it];
    const Index as = a_ptr[r], la = a_ptr[r + 1] - as;
    const Index bs = tt.beg[r], lb = tt.end[r] - bs;   // (a binned row is in the region: bs >= 0)
    long long d0 = 0, d1 = (long long)la + lb;
    if (seg_k) {
      d0 = (long long)seg_k[it] * kASeg;
      d1 = d1 < d0 + kASeg ? d1 : d0 + kASeg;
    }
    // merge path: i0 = the A elements among the first d0 merged (ties: A first)
    Index i0 = 0;
    if (d0 > 0) {
      Index lo = d0 > lb ? (Index)(d0 - lb) : 0, hi = d0 < la ? (Index)d0 : la;
      while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if ((unsigned int)a_ind[as + mid] <= am_tcol(tt, bs + (Index)(d0 - 1 - mid))) lo = mid + 1; else hi = mid;
      }
      i0 = lo;
    }
    Index j0 = (Index)(d0 - i0);
    unsigned int prev_a = i0 > 0 ? (unsigned int)a_ind[as + i0 - 1] : kANone;
    Index ms = 0, me = 0;
    if (m_ptr) { ms = m_ptr[r]; me = m_ptr[r + 1]; }
    Index out = 0;
    if constexpr (kNum) out = seg_k ? c_ptr[r] + (Index)(seg_off[it] - seg_off[it - seg_k[it]]) : c_ptr[r];
    unsigned int cnt = 0;
    for (long long d = d0; d < d1;) {
      const int lim = d1 - d < G ? (int)(d1 - d) : G;
      unsigned int av = kANone, bv = kANone, aval = 0, bval = 0;
      if (i0 + t < la) {
        av = (unsigned int)a_ind[as + i0 + t];
        if constexpr (kNum) aval = a_val[as + i0 + t];
      }
      if (j0 + t < lb) {
        bv = am_tcol(tt, bs + j0 + t);
        if constexpr (kNum) bval = tt.val ? tt.val[bs + j0 + t] : tt.cbits;
      }
      s_a[g0 + t] = av;
      s_b[g0 + t] = bv;
      wave_lds_sync();
      int rb = 0, ra = 0;                              // # B window < av, # A window <= bv
#pragma unroll
      for (int s = G / 2; s > 0; s >>= 1) {
        if (s_b[g0 + rb + s - 1] < av) rb += s;
        if (s_a[g0 + ra + s - 1] <= bv) ra += s;
      }
      if (s_b[g0 + rb] < av) ++rb;                     // (the search above covers ranks 0 .. G - 1)
      if (s_a[g0 + ra] <= bv) ++ra;
      const bool in_a = av != kANone && t + rb < lim;
      const bool in_b = bv != kANone && t + ra < lim;
      const bool pair_a = rb < G && s_b[g0 + rb] == av;             // the owner of a pair
      const bool dup_b = bv == (ra > 0 ? s_a[g0 + ra - 1] : prev_a);  // its partner
      unsigned int partner = 0;
      if constexpr (kNum) partner = (unsigned int)__shfl((int)bval, (lane & ~(G - 1)) + (rb & (G - 1)), kWave);
      const int n_a = __popcll(__ballot(in_a) & gmask);
      const unsigned int last_a = n_a > 0 ? s_a[g0 + n_a - 1] : prev_a;
      wave_lds_sync();
      if (in_a) {
        s_col[g0 + t + rb] = av;
        s_kind[g0 + t + rb] = pair_a ? 1 : 0;
        if constexpr (kNum) {
          s_c[g0 + t + rb] = aval;
          s_z[g0 + t + rb] = !pair_a ? aval : accum < 0 ? partner : am_bits(binop_rt<T>(accum, am_from<T>(aval), am_from<T>(partner)));
        }
      }
      if (in_b) {
        s_col[g0 + t + ra] = dup_b ? kANone : bv;
        s_kind[g0 + t + ra] = 2;
        if constexpr (kNum) s_z[g0 + t + ra] = bval;
      }
      wave_lds_sync();
      const unsigned int col = t < lim ? s_col[g0 + t] : kANone;
      const int kind = s_kind[g0 + t];
      bool keep = col != kANone, use_z = true;
      if (keep) {
        // what Z holds here: an entry of the old C alone survives outside J, or under an accum
        bool zkeep = true;
        if (kind == 0 && accum < 0) zkeep = tt.cptr && !(tt.cptr[col + 1] > tt.cptr[col]);
        const bool differs = kind == 2 || (kind == 0 && !zkeep) || (kind == 1 && kNum);   // Z and the old C differ here
        bool pass = true;
        if (m_ptr && differs) {
          Index lo = ms, hi = me;
          while (lo < hi) {
            const Index mid = lo + ((hi - lo) >> 1);
            if ((unsigned int)m_ind[mid] < col) lo = mid + 1; else hi = mid;
          }
          const bool present = lo < me && (unsigned int)m_ind[lo] == col && mask_nonzero(m_val, mask_f32, lo);
          pass = present != (scmp != 0);
        }
        if (kind == 0) keep = zkeep || !pass;
        else if (kind == 2) keep = pass;
        else use_z = pass;
      }
      const unsigned long long km = __ballot(keep) & gmask;
      if constexpr (kNum) {
        if (keep) {
          const Index pos = out + (Index)__popcll(km & below);
          c_ind[pos] = (Index)col;
          c_val[pos] = use_z ? s_z[g0 + t] : s_c[g0 + t];
        }
        out += (Index)__popcll(km);
      }
      cnt += (unsigned int)__popcll(km);
      i0 += n_a;
      j0 += lim - n_a;
      prev_a = last_a;
      d += lim;
      wave_lds_sync();
    }
    if constexpr (!kNum) {
      if (t == 0) {
        if (!seg_k) counts[r] = cnt;
        else {
          seg_cnt[it] = cnt;
          if (cnt) atomicAdd(&counts[r], cnt);         // (integers: the sum does not depend on the order)
        }
      }
    }
  }
}

// the copied rows: entry p of the old C finds its row by binary search and moves by the row's shift
__global__ __launch_bounds__(kBlock) void am_copy_kernel(const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                         const unsigned int* __restrict__ a_val, Index m, Index nnz, AmT t, int accum,
                                                         const Index* __restrict__ c_ptr, Index* __restrict__ c_ind,
                                                         unsigned int* __restrict__ c_val) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) {
    Index lo = 0, hi = m;                              // the row: the last r with a_ptr[r] <= p
    while (hi - lo > 1) {
      const Index mid = lo + ((hi - lo) >> 1);
      if (a_ptr[mid] <= (Index)p) lo = mid; else hi = mid;
    }
    if (!am_is_copy(t, lo, accum)) continue;
    const Index pos = c_ptr[lo] + ((Index)p - a_ptr[lo]);
    c_ind[pos] = a_ind[p];
    c_val[pos] = a_val[p];
  }
}

namespace {

// T of one orientation and the device memory behind it
struct TBuf {
  EwmBuf range, ind, pairs;
  AmT t = {nullptr, nullptr, nullptr, nullptr, 0u, nullptr};
};

// a list without repeats: inverted, and GRB_INVALID_INDEX when an index occurs twice
grb_info list_unique(IndexList* L) {
  if (!L->host) return GRB_SUCCESS;
  hipStream_t s = ctx().stream;
  GRB_TRY(list_invert(L));
  if (L->n < 2) return GRB_SUCCESS;
  EwmBuf flag;
  GRB_TRY(ewm_alloc(&flag, 4));
  GRB_HIP_TRY(hipMemsetAsync(flag.p, 0, 4, s));
  hipLaunchKernelGGL(am_dup_kernel, dim3(stream_grid(L->dim, kBlock)), dim3(kBlock), 0, s, L->jptr(), L->dim, (unsigned int*)flag.p);
  GRB_HIP_TRY(hipGetLastError());
  unsigned int dup = 0;
  GRB_HIP_TRY(hipMemcpyAsync(&dup, flag.p, 4, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  return dup ? GRB_INVALID_INDEX : GRB_SUCCESS;
}

grb_info t_alloc_range(TBuf* b, Index m) {
  GRB_TRY(ewm_alloc(&b->range, 8 * (size_t)(m > 0 ? m : 1)));
  b->t.beg = (const Index*)b->range.p;
  b->t.end = b->t.beg + m;
  return GRB_SUCCESS;
}

// n (row << 32 | column, value bits) pairs in b->pairs -> sorted, columns unpacked, the rows' ranges found
grb_info t_from_pairs(TBuf* b, Index n, Index m, Index ncols, const IndexList* R) {
  hipStream_t s = ctx().stream;
  const size_t cap = (size_t)(n > 0 ? n : 1);
  unsigned long long* keys = (unsigned long long*)b->pairs.p;
  unsigned int* pay = (unsigned int*)(keys + cap);
  GRB_TRY(device_sort_pairs(keys, pay, n, index_bits(ncols), index_bits(m)));
  GRB_TRY(ewm_alloc(&b->ind, 4 * cap));
  GRB_TRY(t_alloc_range(b, m));
  if (n > 0) {
    hipLaunchKernelGGL(am_unpack_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, keys, n, (Index*)b->ind.p);
    GRB_HIP_TRY(hipGetLastError());
  }
  if (m > 0) {
    hipLaunchKernelGGL(am_keyrange_kernel, dim3(stream_grid(m, kBlock)), dim3(kBlock), 0, s, m, keys, n, R->jptr(), (Index*)b->t.beg,
                       (Index*)b->t.end);
    GRB_HIP_TRY(hipGetLastError());
  }
  b->t.ind = (const Index*)b->ind.p;
  b->t.val = pay;
  return GRB_SUCCESS;
}

// T of C(R, Cl) = X, X one orientation of op(A) (R->n rows); C has m rows and ncols columns in this orientation
grb_info t_matrix(const CsrArrays& X, IndexList* R, IndexList* Cl, Index m, Index ncols, TBuf* b) {
  hipStream_t s = ctx().stream;
  const Index nnz = X.nvals;
  b->t.cptr = Cl->jptr();
  if (Cl->sorted) {
    GRB_TRY(t_alloc_range(b, m));
    if (m > 0) {
      hipLaunchKernelGGL(am_rowrange_kernel, dim3(stream_grid(m, kBlock)), dim3(kBlock), 0, s, m, R->jptr(), R->jpos(), X.ptr, 0,
                         (Index*)b->t.beg, (Index*)b->t.end);
      GRB_HIP_TRY(hipGetLastError());
    }
    b->t.ind = X.ind;
    if (Cl->host) {
      GRB_TRY(ewm_alloc(&b->ind, 4 * (size_t)(nnz > 0 ? nnz : 1)));
      if (nnz > 0) {
        hipLaunchKernelGGL(am_mapcols_kernel, dim3(stream_grid(nnz, kBlock)), dim3(kBlock), 0, s, X.ind, nnz, Cl->dev(), (Index*)b->ind.p);
        GRB_HIP_TRY(hipGetLastError());
      }
      b->t.ind = (const Index*)b->ind.p;
    }
    b->t.val = (const unsigned int*)X.val;
    return GRB_SUCCESS;
  }
  // J in no order: (row, column) keys, sorted over the bits the two dimensions need
  const size_t cap = (size_t)(nnz > 0 ? nnz : 1);
  GRB_TRY(ewm_alloc(&b->pairs, 12 * cap));
  if (nnz > 0) {
    unsigned long long* keys = (unsigned long long*)b->pairs.p;
    hipLaunchKernelGGL(am_keys_kernel, dim3(stream_grid(nnz, kBlock)), dim3(kBlock), 0, s, X.ptr, X.ind, (const unsigned int*)X.val, R->n,
                       nnz, R->dev(), Cl->dev(), keys, (unsigned int*)(keys + cap));
    GRB_HIP_TRY(hipGetLastError());
  }
  return t_from_pairs(b, nnz, m, ncols, R);
}

// T of the row / column form in one orientation: u's stored entries at (L[k], fixed) (list_major) or (fixed, L[k])
grb_info t_vector(grb_vector u, IndexList* L, Index fixed, bool list_major, IndexList* R, IndexList* Cl, Index m, Index ncols, TBuf* b) {
  hipStream_t s = ctx().stream;
  const bool sparse = u->vec_type == GRB_SPARSE;
  const Index nu = sparse ? u->s_nvals : u->nsize;
  b->t.cptr = Cl->jptr();
  const size_t cap = (size_t)(nu > 0 ? nu : 1);
  GRB_TRY(ewm_alloc(&b->pairs, 12 * cap));
  if (nu > 0) {
    unsigned long long* keys = (unsigned long long*)b->pairs.p;
    hipLaunchKernelGGL(am_vec_keys_kernel, dim3(stream_grid(nu, kBlock)), dim3(kBlock), 0, s, sparse ? u->s_ind : nullptr,
                       (const unsigned int*)(sparse ? u->s_val : u->d_val), nu, L->dev(), fixed, list_major ? 1 : 0, keys,
                       (unsigned int*)(keys + cap));
    GRB_HIP_TRY(hipGetLastError());
  }
  return t_from_pairs(b, nu, m, ncols, R);
}

// T of the constant form: every row of R is the ascending copy of Cl
grb_info t_constant(unsigned int cbits, IndexList* R, IndexList* Cl, Index m, TBuf* b) {
  hipStream_t s = ctx().stream;
  b->t.cptr = Cl->jptr();
  b->t.cbits = cbits;
  GRB_TRY(t_alloc_range(b, m));
  if (m > 0) {
    hipLaunchKernelGGL(am_rowrange_kernel, dim3(stream_grid(m, kBlock)), dim3(kBlock), 0, s, m, R->jptr(), R->jpos(), nullptr, Cl->n,
                       (Index*)b->t.beg, (Index*)b->t.end);
    GRB_HIP_TRY(hipGetLastError());
  }
  if (Cl->host) {
    GRB_TRY(ewm_alloc(&b->ind, 4 * (size_t)(Cl->n > 0 ? Cl->n : 1)));
    if (Cl->n > 0) {
      hipLaunchKernelGGL(am_selcols_kernel, dim3(stream_grid(Cl->dim, kBlock)), dim3(kBlock), 0, s, Cl->jptr(), Cl->dim, (Index*)b->ind.p);
      GRB_HIP_TRY(hipGetLastError());
    }
    b->t.ind = (const Index*)b->ind.p;
  }
  return GRB_SUCCESS;
}

template <typename T, bool kNum>
grb_info launch_merge(hipStream_t s, const RowBins& b, const CsrArrays& X, const AmT& t, const CsrArrays* M, int mask_f32, int scmp,
                      int accum, unsigned int* counts, const Index* c_ptr, Index* c_ind, unsigned int* c_val) {
  const Index* mp = M ? M->ptr : nullptr;
  const Index* mi = M ? M->ind : nullptr;
  const void* mv = M ? M->val : nullptr;
  return for_each_bin<kAShort>(b, [&](auto g, int grid, const Index* items, const Index* seg_k, Index n) {
    unsigned int* seg_cnt = seg_k ? b.seg_cnt : nullptr;   // a segment's count (kNum = false), then its offset
    hipLaunchKernelGGL((am_merge_kernel<T, decltype(g)::value, kNum>), dim3(grid), dim3(kBlock), 0, s, items, seg_k, n, X.ptr, X.ind,
                       (const unsigned int*)X.val, t, mp, mi, mv, mask_f32, scmp, accum, counts, seg_cnt, c_ptr, seg_cnt, c_ind, c_val);
  });
}

// one orientation: the m rows of the old C (X) merged with T under the mask's rows (M, nullable) -> out
grb_info assign_side(int dtype, const CsrArrays& X, Index m, const AmT& t, const CsrArrays* M, int mask_f32, int scmp, int accum,
                     Side* out) {
  hipStream_t s = ctx().stream;
  const AmRowLen len_of{X.ptr, t, accum};
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)m + 1)));
  unsigned int* counts = (unsigned int*)out->ptr.p;
  GRB_HIP_TRY(hipMemsetAsync(counts, 0, 4 * ((size_t)m + 1), s));
  RowBins b;
  GRB_TRY(row_bins_head(&b, s));
  if (m > 0) {
    hipLaunchKernelGGL(am_len_kernel, dim3(stream_grid(m, kBlock * 8)), dim3(kBlock), 0, s, len_of, m, counts, b.d_tot);
    GRB_HIP_TRY(hipGetLastError());
  }
  GRB_TRY(row_bins_sized(&b, m, s));
  if (m > 0 && (b.nbin[0] || b.nbin[1] || b.nbin[2])) GRB_TRY((row_bins_fill<2 * kAShort, kASeg>(b, len_of, m, s)));
  // ---- symbolic (value-free: one instantiation serves both types)
  GRB_TRY((launch_merge<float, false>(s, b, X, t, M, mask_f32, scmp, accum, counts, nullptr, nullptr, nullptr)));
  GRB_TRY(row_bins_total(b, counts, m, false, s, out));  // (the merge kernel has added the hub segments into their rows)
  GRB_TRY(row_bins_pointers(b, m, out));
  if (out->nnz == 0) return GRB_SUCCESS;
  // ---- numeric
  const Index* cp = (const Index*)counts;
  Index* ci = (Index*)out->ind.p;
  unsigned int* cv = (unsigned int*)out->val.p;
  if (b.own > 0) {                                       // the copied rows' entries
    hipLaunchKernelGGL(am_copy_kernel, dim3(stream_grid(X.nvals, kBlock)), dim3(kBlock), 0, s, X.ptr, X.ind, (const unsigned int*)X.val, m,
                       X.nvals, t, accum, cp, ci, cv);
    GRB_HIP_TRY(hipGetLastError());
  }
  if (dtype == GRB_F32) GRB_TRY((launch_merge<float, true>(s, b, X, t, M, mask_f32, scmp, accum, nullptr, cp, ci, cv)));
  else GRB_TRY((launch_merge<int, true>(s, b, X, t, M, mask_f32, scmp, accum, nullptr, cp, ci, cv)));
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // (the lists are freed on the way out)
  return GRB_SUCCESS;
}


// what every form checks first, and the old C's two orientations (an unbuilt C is an empty matrix)
struct OldC {
  CsrArrays r, c;
  EwmBuf zeros;
  bool has_c = false;
};
grb_info old_c(grb_matrix C, OldC* o) {
  if (C->built && C->csr.ptr) {
    o->r = C->csr;
    o->has_c = has_csc(C);
    if (o->has_c) o->c = C->csc;
    return GRB_SUCCESS;
  }
  const Index big = C->nrows > C->ncols ? C->nrows : C->ncols;
  GRB_TRY(ewm_alloc(&o->zeros, 4 * ((size_t)big + 1)));
  GRB_HIP_TRY(hipMemsetAsync(o->zeros.p, 0, 4 * ((size_t)big + 1), ctx().stream));
  o->r.ptr = o->c.ptr = (Index*)o->zeros.p;
  o->r.n = C->nrows;
  o->c.n = C->ncols;
  o->has_c = true;
  return GRB_SUCCESS;
}
grb_info check_types(grb_matrix C, grb_matrix mask, int src_dtype, int accum_op) {
  if ((C->dtype != GRB_F32 && C->dtype != GRB_I32) || src_dtype != C->dtype) return GRB_NOT_IMPLEMENTED;
  if (mask && mask->dtype != GRB_F32 && mask->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  if (accum_op >= (int)GRB_N_BINARY_OPS) return GRB_INVALID_VALUE;
  if (mask && (mask->nrows != C->nrows || mask->ncols != C->ncols)) return GRB_DIMENSION_MISMATCH;
  return GRB_SUCCESS;
}

}  // namespace

grb_info assign_matrix(grb_matrix C, grb_matrix mask, int accum_op, grb_matrix A, const Index* rows, Index nrows, const Index* cols,
                       Index ncols, bool tran, bool scmp) {
  GRB_TRY(check_types(C, mask, A->dtype, accum_op));
  const Index am = tran ? A->ncols : A->nrows, an = tran ? A->nrows : A->ncols;   // op(A) is am x an
  if (nrows != am || ncols != an) return GRB_DIMENSION_MISMATCH;
  IndexList I, J;
  GRB_TRY(list_check(&I, rows, nrows, C->nrows));
  GRB_TRY(list_check(&J, cols, ncols, C->ncols));
  if ((tran && !has_csc(A)) || !A->csr.ptr || (mask && !mask->csr.ptr)) return GRB_INVALID_OBJECT;
  GRB_TRY(list_unique(&I));
  GRB_TRY(list_unique(&J));
  OldC o;
  GRB_TRY(old_c(C, &o));
  const CsrArrays& Xr = tran ? A->csc : A->csr;          // rows of op(A)
  const CsrArrays& Xc = tran ? A->csr : A->csc;          // its columns
  const bool both = C->format != 1 && o.has_c && (tran || has_csc(A)) && (!mask || has_csc(mask));
  const int mask_f32 = mask && mask->dtype == GRB_F32 ? 1 : 0;
  const int acc = accum_op < 0 ? -1 : accum_op;
  Side r, c;
  {
    TBuf t;
    GRB_TRY(t_matrix(Xr, &I, &J, C->nrows, C->ncols, &t));
    GRB_TRY(assign_side(C->dtype, o.r, C->nrows, t.t, mask ? &mask->csr : nullptr, mask_f32, scmp ? 1 : 0, acc, &r));
  }
  if (both) {
    TBuf t;
    GRB_TRY(t_matrix(Xc, &J, &I, C->ncols, C->nrows, &t));
    GRB_TRY(assign_side(C->dtype, o.c, C->ncols, t.t, mask ? &mask->csc : nullptr, mask_f32, scmp ? 1 : 0, acc, &c));
  }
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));       // (the lists are the caller's; A or the mask may be C)
  return attach(C, &r, both ? &c : nullptr);
}

grb_info assign_matrix_scalar(grb_matrix C, grb_matrix mask, int accum_op, double val, const Index* rows, Index nrows,
                              const Index* cols, Index ncols, bool scmp) {
  GRB_TRY(check_types(C, mask, C->dtype, accum_op));
  IndexList I, J;
  GRB_TRY(list_check(&I, rows, nrows, C->nrows));
  GRB_TRY(list_check(&J, cols, ncols, C->ncols));
  if (mask && !mask->csr.ptr) return GRB_INVALID_OBJECT;
  // without a mask every position of I x J is stored afterwards: known before anything is allocated
  if (!mask && (long long)nrows * (long long)ncols > (long long)INT32_MAX) return GRB_OUT_OF_MEMORY;
  GRB_TRY(list_unique(&I));
  GRB_TRY(list_unique(&J));
  OldC o;
  GRB_TRY(old_c(C, &o));
  const bool both = C->format != 1 && o.has_c && (!mask || has_csc(mask));
  const int mask_f32 = mask && mask->dtype == GRB_F32 ? 1 : 0;
  const int acc = accum_op < 0 ? -1 : accum_op;
  unsigned int cbits;
  if (C->dtype == GRB_F32) { const float f = (float)val; memcpy(&cbits, &f, 4); }
  else { const int i = (int)val; memcpy(&cbits, &i, 4); }
  Side r, c;
  {
    TBuf t;
    GRB_TRY(t_constant(cbits, &I, &J, C->nrows, &t));
    GRB_TRY(assign_side(C->dtype, o.r, C->nrows, t.t, mask ? &mask->csr : nullptr, mask_f32, scmp ? 1 : 0, acc, &r));
  }
  if (both) {
    TBuf t;
    GRB_TRY(t_constant(cbits, &J, &I, C->ncols, &t));
    GRB_TRY(assign_side(C->dtype, o.c, C->ncols, t.t, mask ? &mask->csc : nullptr, mask_f32, scmp ? 1 : 0, acc, &c));
  }
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return attach(C, &r, both ? &c : nullptr);
}

// is_col: C(list, fixed) = u; else C(fixed, list) = u
grb_info assign_matrix_vector(grb_matrix C, int accum_op, grb_vector u, const Index* list, Index nlist, Index fixed, bool is_col) {
  if (u->vec_type != GRB_SPARSE && u->vec_type != GRB_DENSE) return GRB_UNINITIALIZED_OBJECT;
  GRB_TRY(check_types(C, nullptr, u->dtype, accum_op));
  if (nlist != u->nsize) return GRB_DIMENSION_MISMATCH;
  const Index ldim = is_col ? C->nrows : C->ncols, fdim = is_col ? C->ncols : C->nrows;
  IndexList L, F;
  GRB_TRY(list_check(&L, list, nlist, ldim));
  if (fixed < 0 || fixed >= fdim) return GRB_INDEX_OUT_OF_BOUNDS;
  GRB_TRY(list_check(&F, &fixed, 1, fdim));
  GRB_TRY(list_unique(&L));
  GRB_TRY(list_unique(&F));
  OldC o;
  GRB_TRY(old_c(C, &o));
  const bool both = C->format != 1 && o.has_c;
  const int acc = accum_op < 0 ? -1 : accum_op;
  IndexList* I = is_col ? &L : &F;                       // the region's rows and columns
  IndexList* J = is_col ? &F : &L;
  Side r, c;
  {
    TBuf t;
    GRB_TRY(t_vector(u, &L, fixed, is_col, I, J, C->nrows, C->ncols, &t));
    GRB_TRY(assign_side(C->dtype, o.r, C->nrows, t.t, nullptr, 0, 0, acc, &r));
  }
  if (both) {
    TBuf t;
    GRB_TRY(t_vector(u, &L, fixed, !is_col, J, I, C->ncols, C->nrows, &t));
    GRB_TRY(assign_side(C->dtype, o.c, C->ncols, t.t, nullptr, 0, 0, acc, &c));
  }
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return attach(C, &r, both ? &c : nullptr);
}

}  // namespace grb

using namespace grb;

// assign, matrix forms (operations.hpp:441-551): the contract is the comment in include/grb_hip.h
grb_info grb_matrix_assign(grb_matrix C, grb_matrix mask, int accum_op, grb_matrix A, const grb_index* row_indices, grb_index nrows,
                           const grb_index* col_indices, grb_index ncols, grb_descriptor desc) { GRB_API_ENTER();
  if (!C || !A) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built || (mask && !mask->built)) return GRB_UNINITIALIZED_OBJECT;
  return assign_matrix(C, mask, accum_op, A, row_indices, nrows, col_indices, ncols, desc && desc->desc[GRB_INP0] == GRB_TRAN,
                       desc && desc->desc[GRB_MASK] == GRB_SCMP);
}

grb_info grb_matrix_assign_scalar(grb_matrix C, grb_matrix mask, int accum_op, double val, const grb_index* row_indices,
                                  grb_index nrows, const grb_index* col_indices, grb_index ncols, grb_descriptor desc) { GRB_API_ENTER();
  if (!C) return GRB_UNINITIALIZED_OBJECT;
  if (mask && !mask->built) return GRB_UNINITIALIZED_OBJECT;
  return assign_matrix_scalar(C, mask, accum_op, val, row_indices, nrows, col_indices, ncols, desc && desc->desc[GRB_MASK] == GRB_SCMP);
}

grb_info grb_matrix_assign_col(grb_matrix C, grb_vector mask, int accum_op, grb_vector u, const grb_index* row_indices,
                               grb_index nrows, grb_index col_index, grb_descriptor desc) { GRB_API_ENTER();
  (void)desc;
  if (!C || !u) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return assign_matrix_vector(C, accum_op, u, row_indices, nrows, col_index, true);
}

grb_info grb_matrix_assign_row(grb_matrix C, grb_vector mask, int accum_op, grb_vector u, grb_index row_index,
                               const grb_index* col_indices, grb_index ncols, grb_descriptor desc) { GRB_API_ENTER();
  (void)desc;
  if (!C || !u) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return assign_matrix_vector(C, accum_op, u, col_indices, ncols, row_index, false);
}
