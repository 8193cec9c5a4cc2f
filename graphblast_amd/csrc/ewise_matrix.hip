// ewise_matrix.hip -- the element-wise forms of two matrices (grb_matrix_eWiseAdd: the union of the structures,
// grb_matrix_eWiseMult: the intersection; the reference declares both, operations.hpp:166-204, 307-325, and returns
// GrB_NOT_IMPLEMENTED, backend/cuda/operations.hpp:414-423) and the transposition (grb_transpose, operations.hpp:682).
//
// Element-wise: row i of C is the merge of row i of op(A) and row i of op(B) (two ascending column lists), filtered by
// row i of the mask, in a symbolic pass (counts) and a numeric pass (columns and values) over the same row bins (the bin
// kernel, the launches per bin and the counts-to-pointers tail: row_bins.hpp):
//   bins      len(i) = |row i of op(A)| + |row i of op(B)| (rows of length 0, and for the intersection rows with an empty
//             side, are in no bin: their count stays 0)
//               short  len <= 2 * kShort          a 16-lane group per row (four rows per wave)
//               wave   len <= kSeg                a wave per row
//               hub    the rest                   the row cut into segments of kSeg merged positions, a wave each;
//                                                 a segment's start in both lists is found by a merge-path search
//   merge     a group takes G merged positions per step: it loads the next G columns of each list (a window, coalesced),
//             ranks every element in the other window by binary search in LDS (A: lower bound, B: upper bound, so equal
//             columns put A's first), and an element's merged position is its own index plus that rank.  Positions below
//             G are this step's; the others wait for the next.  An A element equal to a B element is the pair's owner
//             (its partner is in the B window: the rank points at it); the B element is the duplicate (its A partner is
//             in the A window just below its rank, or is the last A column of an earlier step or segment).  Owners
//             carry add(a, b) or mul(a, b); for the union, elements without a partner carry their own value.
//   mask      a kept element is probed in the mask row by binary search (the mask's CSR, or its CSC for C's CSC)
//   output    the step's kept flags, one per merged position, are balloted: prefix counts give every element its slot.
// No atomics on values: a result's bits follow from its two operands alone.  The counts of a hub row's segments are
// added into the row's count (integers) and scanned for the numeric pass's offsets.
//
// Transposition: two device copies when the source orientation exists; otherwise the CSR is sorted into column-major
// order by the stable radix sort of build.hip (key = the column, entries in row-major order: rows stay ascending inside
// every column), the row and value of every entry gathered behind it, and every column's start found by binary search
// in the sorted keys.
#include "row_bins.hpp"

namespace grb {

constexpr int kShort = 16;              // lanes per row of the short bin (rows of at most 2 * kShort merged entries)
constexpr int kSeg = 2048;              // merged positions per wave of the wave and hub bins
constexpr unsigned int kNone = 0xffffffffu;   // no column: above every column index (columns < ncols <= INT32_MAX)

// a row's merged length; the intersection drops rows with an empty side
struct EwmRowLen {
  const Index* a_ptr;
  const Index* b_ptr;
  int intersect;
  __device__ long long operator()(long long i) const {
    const Index la = a_ptr[i + 1] - a_ptr[i], lb = b_ptr[i + 1] - b_ptr[i];
    return intersect && (la == 0 || lb == 0) ? 0 : (long long)(la + lb);
  }
};

// One kernel for every bin: groups of G lanes (G = kShort or kWave), each taking one item at a time -- a whole row
// (seg_k == nullptr) or one kSeg-long segment of a hub row.  kNum = false: counts only.  kAdd: union, else intersection.
template <int SR, typename T, int G, bool kNum, bool kAdd>
__global__ __launch_bounds__(kBlock) void ewm_merge_kernel(const Index* __restrict__ items, const Index* __restrict__ seg_k, Index nitems,
                                                           const Index* __restrict__ a_ptr, const Index* __restrict__ a_ind,
                                                           const T* __restrict__ a_val, const Index* __restrict__ b_ptr,
                                                           const Index* __restrict__ b_ind, const T* __restrict__ b_val,
                                                           const Index* __restrict__ m_ptr, const Index* __restrict__ m_ind,
                                                           const void* __restrict__ m_val, int mask_f32, int scmp,
                                                           unsigned int* __restrict__ counts, unsigned int* __restrict__ seg_cnt,
                                                           const Index* __restrict__ c_ptr, const unsigned int* __restrict__ seg_off,
                                                           Index* __restrict__ c_ind, T* __restrict__ c_val) {
  typedef Semiring<SR, T> S;
  __shared__ unsigned int s_a[kBlock], s_b[kBlock], s_col[kBlock];
  __shared__ T s_val[kNum ? kBlock : 1];
  const int lane = lane_id(), t = lane & (G - 1);
  const int g0 = threadIdx.x - t;                      // the group's first slot in the LDS arrays
  const unsigned long long gmask = G == kWave ? ~0ull : (((1ull << (G % kWave)) - 1ull) << (lane & ~(G - 1)));
  const unsigned long long below = (1ull << lane) - 1ull;
  constexpr int kGroups = kBlock / G;
  const long long step = (long long)gridDim.x * kGroups;
  for (long long it = (long long)blockIdx.x * kGroups + threadIdx.x / G; it < nitems; it += step) {
    const Index r = items[it];
    const Index as = a_ptr[r], la = a_ptr[r + 1] - as;
    const Index bs = b_ptr[r], lb = b_ptr[r + 1] - bs;
    Index d0 = 0, d1 = la + lb;
    if (seg_k) {
      d0 = seg_k[it] * kSeg;
      d1 = d1 < d0 + kSeg ? d1 : d0 + kSeg;
    }
    // merge path: i0 = the A elements among the first d0 merged (ties: A first)
    Index i0 = 0;
    if (d0 > 0) {
      Index lo = d0 > lb ? d0 - lb : 0, hi = d0 < la ? d0 : la;
      while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if (a_ind[as + mid] <= b_ind[bs + d0 - 1 - mid]) lo = mid + 1; else hi = mid;
      }
      i0 = lo;
    }
    Index j0 = d0 - i0;
    unsigned int prev_a = i0 > 0 ? (unsigned int)a_ind[as + i0 - 1] : kNone;
    Index ms = 0, me = 0;
    if (m_ptr) { ms = m_ptr[r]; me = m_ptr[r + 1]; }
    Index out = 0;
    if constexpr (kNum) out = seg_k ? c_ptr[r] + (Index)(seg_off[it] - seg_off[it - seg_k[it]]) : c_ptr[r];
    unsigned int cnt = 0;
    for (Index d = d0; d < d1;) {
      const int lim = d1 - d < G ? (int)(d1 - d) : G;
      unsigned int av = kNone, bv = kNone;
      T aval = T(0), bval = T(0);
      if (i0 + t < la) {
        av = (unsigned int)a_ind[as + i0 + t];
        if constexpr (kNum) aval = a_val[as + i0 + t];
      }
      if (j0 + t < lb) {
        bv = (unsigned int)b_ind[bs + j0 + t];
        if constexpr (kNum) bval = b_val[bs + j0 + t];
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
      const bool in_a = av != kNone && t + rb < lim;
      const bool in_b = bv != kNone && t + ra < lim;
      const bool pair_a = rb < G && s_b[g0 + rb] == av;             // the owner of a pair
      const bool dup_b = bv == (ra > 0 ? s_a[g0 + ra - 1] : prev_a);  // its partner
      T partner = T(0);
      if constexpr (kNum) partner = __shfl(bval, (lane & ~(G - 1)) + (rb & (G - 1)), kWave);
      const int n_a = __popcll(__ballot(in_a) & gmask);
      const unsigned int last_a = n_a > 0 ? s_a[g0 + n_a - 1] : prev_a;
      wave_lds_sync();
      if (in_a) {
        const bool keep = kAdd || pair_a;
        s_col[g0 + t + rb] = keep ? av : kNone;
        if constexpr (kNum) s_val[g0 + t + rb] = pair_a ? (kAdd ? S::add(aval, partner) : S::mul(aval, partner)) : aval;
      }
      if (in_b) {
        s_col[g0 + t + ra] = (kAdd && !dup_b) ? bv : kNone;
        if constexpr (kNum) s_val[g0 + t + ra] = bval;
      }
      wave_lds_sync();
      const unsigned int col = t < lim ? s_col[g0 + t] : kNone;
      bool keep = col != kNone;
      if (m_ptr && keep) {
        const Index p = index_lower_bound(m_ind, ms, me, (Index)col);
        const bool present = p < me && (unsigned int)m_ind[p] == col && mask_nonzero(m_val, mask_f32, p);
        keep = present != (scmp != 0);
      }
      const unsigned long long km = __ballot(keep) & gmask;
      if constexpr (kNum) {
        if (keep) {
          const Index pos = out + (Index)__popcll(km & below);
          c_ind[pos] = (Index)col;
          c_val[pos] = s_val[g0 + t];
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

// ---- transposition of a CSR without its CSC
// key of entry e = (row << 32) | column: the sort orders by the column bits only and keeps row-major order inside a column
__global__ __launch_bounds__(kBlock) void ewm_tr_keys_kernel(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index m,
                                                             Index nvals, unsigned long long* __restrict__ keys,
                                                             unsigned int* __restrict__ pay) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < nvals; e += stride) {
    Index lo = 0, hi = m;                              // the row: the last r with ptr[r] <= e
    while (hi - lo > 1) {
      const Index mid = lo + ((hi - lo) >> 1);
      if (ptr[mid] <= (Index)e) lo = mid; else hi = mid;
    }
    keys[e] = ((unsigned long long)(unsigned int)lo << 32) | (unsigned int)ind[e];
    pay[e] = (unsigned int)e;
  }
}

// sorted keys -> the transpose's row indices (the source rows) and values
__global__ __launch_bounds__(kBlock) void ewm_tr_gather_kernel(const unsigned long long* __restrict__ keys,
                                                               const unsigned int* __restrict__ pay, const unsigned int* __restrict__ val,
                                                               Index nvals, Index* __restrict__ t_ind, unsigned int* __restrict__ t_val) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nvals; p += stride) {
    t_ind[p] = (Index)(keys[p] >> 32);
    t_val[p] = val[pay[p]];
  }
}

// the transpose's pointers: t_ptr[c] = the first sorted entry of column >= c (a search per column, no histogram atomics)
__global__ __launch_bounds__(kBlock) void ewm_tr_ptr_kernel(const unsigned long long* __restrict__ keys, Index nvals, Index n,
                                                            Index* __restrict__ t_ptr) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c <= n; c += stride) {
    Index lo = 0, hi = nvals;
    while (lo < hi) {
      const Index mid = lo + ((hi - lo) >> 1);
      if ((long long)(unsigned int)keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    t_ptr[c] = lo;
  }
}

// (EwmBuf, Side: common.hpp -- extract.hip installs its results the same way)
grb_info ewm_alloc(EwmBuf* b, size_t bytes) {
  if (hipMalloc(&b->p, bytes ? bytes : 4) != hipSuccess) {
    (void)hipGetLastError();                             // (the failed allocation leaves its error behind)
    b->p = nullptr;
    return GRB_OUT_OF_MEMORY;
  }
  return GRB_SUCCESS;
}

namespace {
// no length pass: the call's one work allocation has the lists at their upper bounds (every row, and the segments below),
// carved for the larger of the two orientations
size_t merge_max_segs(long long nvals_a, long long nvals_b) { return (size_t)(2 * (nvals_a + nvals_b) / kSeg + 2); }

// one orientation: m rows of op(A) and op(B) (Aa, Bb), the mask's rows (Mm, nullable) -> out
template <bool kAdd>
grb_info merge_side(int op, int dtype, Index m, const CsrArrays& Aa, const CsrArrays& Bb, const CsrArrays* Mm, int mask_f32,
                    int scmp, RowBins& w, Side* out) {
  hipStream_t s = ctx().stream;
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)m + 1)));
  unsigned int* counts = (unsigned int*)out->ptr.p;
  GRB_HIP_TRY(hipMemsetAsync(counts, 0, 4 * ((size_t)m + 1), s));
  GRB_TRY(row_bins_zero_head(&w, s));
  if (m > 0) GRB_TRY((row_bins_fill<2 * kShort, kSeg>(w, EwmRowLen{Aa.ptr, Bb.ptr, kAdd ? 0 : 1}, m, s)));
  GRB_HIP_TRY(hipMemcpyAsync(w.nbin, w.d_ctr, 12, hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  const Index* mp = Mm ? Mm->ptr : nullptr;
  const Index* mi = Mm ? Mm->ind : nullptr;
  const void* mv = Mm ? Mm->val : nullptr;
  // ---- symbolic (value-free: one instantiation serves every semiring and type)
  GRB_TRY(for_each_bin<kShort>(w, [&](auto g, int grid, const Index* items, const Index* seg_k, Index n) {
    hipLaunchKernelGGL((ewm_merge_kernel<GRB_PLUS_MULTIPLIES, float, decltype(g)::value, false, kAdd>), dim3(grid), dim3(kBlock), 0, s, items,
                       seg_k, n, Aa.ptr, Aa.ind, (const float*)Aa.val, Bb.ptr, Bb.ind, (const float*)Bb.val, mp, mi, mv, mask_f32, scmp,
                       counts, seg_k ? w.seg_cnt : nullptr, nullptr, nullptr, nullptr, nullptr);
  }));
  GRB_TRY(row_bins_total(w, counts, m, false, s, out));  // (the merge kernel has added the hub segments into their rows)
  GRB_TRY(row_bins_pointers(w, m, out));
  if (out->nnz == 0) return GRB_SUCCESS;
  // ---- numeric
  return dispatch_semiring(op, dtype, [&](auto tag, auto tv) -> grb_info {
    using T = decltype(tv);
    constexpr int SR = decltype(tag)::value;
    return for_each_bin<kShort>(w, [&](auto g, int grid, const Index* items, const Index* seg_k, Index n) {
      hipLaunchKernelGGL((ewm_merge_kernel<SR, T, decltype(g)::value, true, kAdd>), dim3(grid), dim3(kBlock), 0, s, items, seg_k, n, Aa.ptr,
                         Aa.ind, (const T*)Aa.val, Bb.ptr, Bb.ind, (const T*)Bb.val, mp, mi, mv, mask_f32, scmp, nullptr, nullptr,
                         (const Index*)counts, seg_k ? w.seg_cnt : nullptr, (Index*)out->ind.p, (T*)out->val.p);
    });
  });
}

}  // namespace

// an orientation is usable when it is there and is not the CSR-only format's alias of the CSR
bool has_csc(const grb_matrix_s* X) { return X->csc.ptr && !X->csc_alias; }

// C is replaced: owned arrays, the host copies of the pointers, the CSR plan built at first use, the CSC plan now
grb_info attach(grb_matrix C, Side* r, Side* c) {
  SpmvPlan plan_csc;
  if (c) GRB_TRY(build_spmv_plan(c->h_ptr, C->ncols, C->nrows, &plan_csc));
  matrix_release_device(C);
  C->owned = true;
  C->nvals = r->nnz;
  C->csr.ptr = (Index*)r->ptr.release();
  C->csr.ind = (Index*)r->ind.release();
  C->csr.val = r->val.release();
  C->csr.n = C->nrows;
  C->csr.nvals = r->nnz;
  C->h_csr_ptr.swap(r->h_ptr);
  C->h_csr_ind.clear(); C->h_csr_val.clear();
  C->h_csc_ptr.clear(); C->h_csc_ind.clear(); C->h_csc_val.clear();
  if (c) {
    C->csc.ptr = (Index*)c->ptr.release();
    C->csc.ind = (Index*)c->ind.release();
    C->csc.val = c->val.release();
    C->csc.n = C->ncols;
    C->csc.nvals = c->nnz;
    C->h_csc_ptr.swap(c->h_ptr);
    C->plan_csc = plan_csc;
  }
  C->nonneg_values = -1; C->mean_value = -1.0; C->small_int_values = -1;
  C->plan_csr_pending = true;
  C->built = true;
  return matrix_apply_format(C);                       // the CSR-only format: the CSC aliases the CSR
}

grb_info ewise_matrix(grb_matrix C, grb_matrix mask, int op, grb_matrix A, grb_matrix B, bool tran_a, bool tran_b, bool scmp,
                      bool add) {
  if (!(A->dtype == GRB_F32 || A->dtype == GRB_I32) || B->dtype != A->dtype || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  if (mask && mask->dtype != GRB_F32 && mask->dtype != GRB_I32) return GRB_NOT_IMPLEMENTED;
  const Index m = tran_a ? A->ncols : A->nrows, n = tran_a ? A->nrows : A->ncols;
  const Index mb = tran_b ? B->ncols : B->nrows, nb = tran_b ? B->nrows : B->ncols;
  if (mb != m || nb != n || C->nrows != m || C->ncols != n) return GRB_DIMENSION_MISMATCH;
  if (mask && (mask->nrows != m || mask->ncols != n)) return GRB_DIMENSION_MISMATCH;
  if ((tran_a && !has_csc(A)) || (tran_b && !has_csc(B)) || !A->csr.ptr || !B->csr.ptr || (mask && !mask->csr.ptr))
    return GRB_INVALID_OBJECT;
  if (op >= GRB_USER_SEMIRING_BASE) {
    UserSemiring u;
    if (!user_semiring_lookup(op, &u)) return GRB_INVALID_VALUE;
  } else if (op < 0 || op >= GRB_N_SEMIRINGS) {
    return GRB_INVALID_VALUE;
  }
  const CsrArrays& Ar = tran_a ? A->csc : A->csr;        // rows of op(A)
  const CsrArrays& Br = tran_b ? B->csc : B->csr;
  // C's CSC: the same merge over the other orientations, when every input has it (and C is not CSR only)
  const bool both = C->format != 1 && (tran_a ? true : has_csc(A)) && (tran_b ? true : has_csc(B)) && (!mask || has_csc(mask));
  const CsrArrays& Ac = tran_a ? A->csr : A->csc;
  const CsrArrays& Bc = tran_b ? B->csr : B->csc;
  const int mask_f32 = mask ? (mask->dtype == GRB_F32 ? 1 : 0) : 0;
  const size_t segs = merge_max_segs(A->nvals, B->nvals);
  const size_t rows = (size_t)(both && n > m ? n : m);
  RowBins w;
  GRB_TRY(row_bins_carve(&w, rows, rows, segs, (rows > segs ? rows : segs) + 1));
  Side r, c;
  auto run = [&](Index rows, const CsrArrays& X, const CsrArrays& Y, const CsrArrays* M, Side* out) {
    return add ? merge_side<true>(op, A->dtype, rows, X, Y, M, mask_f32, scmp ? 1 : 0, w, out)
               : merge_side<false>(op, A->dtype, rows, X, Y, M, mask_f32, scmp ? 1 : 0, w, out);
  };
  GRB_TRY(run(m, Ar, Br, mask ? &mask->csr : nullptr, &r));
  if (both) GRB_TRY(run(n, Ac, Bc, mask ? &mask->csc : nullptr, &c));
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return attach(C, &r, both ? &c : nullptr);
}

namespace {
// a device copy of one orientation
grb_info copy_side(const CsrArrays& X, Index rows, Side* out) {
  hipStream_t s = ctx().stream;
  out->nnz = X.nvals;
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)rows + 1)));
  GRB_TRY(ewm_alloc(&out->ind, 4 * (size_t)(X.nvals > 0 ? X.nvals : 1)));
  GRB_TRY(ewm_alloc(&out->val, 4 * (size_t)(X.nvals > 0 ? X.nvals : 1)));
  GRB_HIP_TRY(hipMemcpyAsync(out->ptr.p, X.ptr, 4 * ((size_t)rows + 1), hipMemcpyDeviceToDevice, s));
  if (X.nvals > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(out->ind.p, X.ind, 4 * (size_t)X.nvals, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemcpyAsync(out->val.p, X.val, 4 * (size_t)X.nvals, hipMemcpyDeviceToDevice, s));
  }
  out->h_ptr.resize((size_t)rows + 1);
  GRB_HIP_TRY(hipMemcpyAsync(out->h_ptr.data(), out->ptr.p, 4 * ((size_t)rows + 1), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  return GRB_SUCCESS;
}

// the transpose of an m x n CSR (n rows of the result) on the device
grb_info sort_side(const CsrArrays& X, Index m, Index n, Side* out) {
  hipStream_t s = ctx().stream;
  const Index nv = X.nvals;
  out->nnz = nv;
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)n + 1)));
  GRB_TRY(ewm_alloc(&out->ind, 4 * (size_t)(nv > 0 ? nv : 1)));
  GRB_TRY(ewm_alloc(&out->val, 4 * (size_t)(nv > 0 ? nv : 1)));
  EwmBuf work;
  GRB_TRY(ewm_alloc(&work, 12 * (size_t)nv));
  unsigned long long* keys = (unsigned long long*)work.p;
  unsigned int* pay = (unsigned int*)(keys + nv);
  if (nv > 0) {
    hipLaunchKernelGGL(ewm_tr_keys_kernel, dim3(stream_grid(nv, kBlock)), dim3(kBlock), 0, s, X.ptr, X.ind, m, nv, keys, pay);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_sort_pairs_range(keys, pay, nv, 0, index_bits(n)));
    hipLaunchKernelGGL(ewm_tr_gather_kernel, dim3(stream_grid(nv, kBlock)), dim3(kBlock), 0, s, keys, pay,
                       (const unsigned int*)X.val, nv, (Index*)out->ind.p, (unsigned int*)out->val.p);
    GRB_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ewm_tr_ptr_kernel, dim3(stream_grid((long long)n + 1, kBlock)), dim3(kBlock), 0, s, keys, nv, n,
                     (Index*)out->ptr.p);
  GRB_HIP_TRY(hipGetLastError());
  out->h_ptr.resize((size_t)n + 1);
  GRB_HIP_TRY(hipMemcpyAsync(out->h_ptr.data(), out->ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  return GRB_SUCCESS;
}
}  // namespace

// ... for a result that has only its CSR so far (contract.hip)
grb_info transpose_side(const CsrArrays& X, Index m, Index n, Side* out) { return sort_side(X, m, n, out); }

grb_info transpose_matrix(grb_matrix C, grb_matrix A, bool tran) {
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  const Index m = tran ? A->nrows : A->ncols, n = tran ? A->ncols : A->nrows;   // C is m x n
  if (C->nrows != m || C->ncols != n) return GRB_DIMENSION_MISMATCH;
  if (!A->csr.ptr) return GRB_INVALID_OBJECT;
  const bool a_csc = has_csc(A);
  const bool both = C->format != 1;
  Side r, c;
  // C's CSR holds the rows of op(A)^T: A's CSC (C = A^T) or A's CSR (C = A); C's CSC the other one
  if (!tran) {
    GRB_TRY(a_csc ? copy_side(A->csc, m, &r) : sort_side(A->csr, A->nrows, A->ncols, &r));
    if (both) GRB_TRY(copy_side(A->csr, n, &c));
  } else {
    GRB_TRY(copy_side(A->csr, m, &r));
    if (both) GRB_TRY(a_csc ? copy_side(A->csc, n, &c) : sort_side(A->csr, A->nrows, A->ncols, &c));
  }
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return attach(C, &r, both ? &c : nullptr);
}

}  // namespace grb
