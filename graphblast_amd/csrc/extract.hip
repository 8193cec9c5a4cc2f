// extract.hip -- the three extract forms (operations.hpp:355-410: subvector, submatrix, matrix column; the reference
// declares them, prints "not implemented yet" and returns GrB_NOT_IMPLEMENTED): grb_matrix_extract, grb_matrix_extract_col,
// grb_vector_extract.  The contract is the comment in include/grb_hip.h.
//
// Submatrix C = X(I, J), X one orientation of op(A): a gather of the rows I[i] with their columns filtered and renumbered.
//   columns   the inverse of J, built once per call: jptr[c] .. jptr[c + 1] are the places of source column c in J (a
//             histogram of J and an exclusive scan), so a source entry yields jptr[c + 1] - jptr[c] output entries:
//             none when c is not selected, several when J repeats it.  A non-decreasing J (found on the host while the
//             list is validated) needs nothing more: those places ARE the output columns, and a row's output comes out
//             ascending.  Any other J also gets jpos[] (the places filled in through per-column cursors, in no fixed
//             order) and the result is ordered afterwards.  A null J is the identity: nothing is built.
//   bins      output rows by the length of their source row (the shared pipeline of row_bins.hpp):
//               short  len <= kXShort   a 16-lane group per row, one step (four rows per wave)
//               wave   len <= kXSeg     a wave per row
//               hub    the rest         the row cut into segments of kXSeg source entries, a wave each
//             A first pass counts the bins' sizes (an output row appears once per occurrence in I, so nothing bounds
//             them beforehand) and the source entries selected; the lists are allocated for exactly that.
//   symbolic  every lane sums the output entries of its source entries; the group's sum is the row's (segment's) count.
//             The counts' 64-bit total is checked against INT32_MAX before anything of C is allocated; the hub rows'
//             segment counts are folded into their rows, and both arrays are scanned into offsets.
//   numeric   a group takes G source entries per step; the inclusive prefix of the lanes' output counts (data-parallel
//             primitives inside the 16-lane row, two row broadcasts for the wave) gives every lane its first slot, and it
//             writes its entries there.  No atomics touch the output: it depends on the inputs alone.
//   order     only when J is not non-decreasing: the numeric pass writes (row << 32 | column, value bits) pairs, the
//             radix sort of build.hip orders them over the significant bits, and they are unpacked.
// C's CSC is the same routine on X's other orientation with I and J exchanged.
//
// Column w = X(I, j) and subvector w = u(I): one ascending (index, value) list -- row j of the orientation, or the sparse
// u -- is probed by binary search for every I[k]; the hits are flagged, scanned and written in order.  A dense u is a gather.
#include "row_bins.hpp"

namespace grb {

constexpr int kXShort = 16;             // the longest source row of the short bin: one step of a 16-lane group
constexpr int kXSeg = 1024;             // the longest source row of the wave bin; source entries per segment of a hub row
constexpr unsigned int kXSat = 0x80000000u;   // a count that large is stored as this: the total then fails the INT32_MAX check

// an output row's length for the bins: that of its source row
struct XtRowLen {
  const Index* sel;                     // nullptr: output row i is source row i
  const Index* x_ptr;
  __device__ long long operator()(long long i) const {
    const Index r = sel ? sel[i] : (Index)i;
    return x_ptr[r + 1] - x_ptr[r];
  }
};

// inclusive prefix sum inside every 16-lane row of the wave (the first five steps of wave_incl_scan_u32)
__device__ __forceinline__ unsigned row_incl_scan_u32(unsigned v) {
  unsigned t = v + __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false)
                 + __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false)
                 + __builtin_amdgcn_update_dpp(0u, v, 0x113, 0xf, 0xf, false);
  t += __builtin_amdgcn_update_dpp(0u, t, 0x114, 0xf, 0xe, false);
  t += __builtin_amdgcn_update_dpp(0u, t, 0x118, 0xf, 0xc, false);
  return t;
}

// ---- the inverse of a list: a histogram (scanned by the caller) and, for a list in no order, the places
__global__ __launch_bounds__(kBlock) void xt_hist_kernel(const Index* __restrict__ list, Index n, unsigned int* __restrict__ hist) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) atomicAdd(&hist[list[k]], 1u);
}
__global__ __launch_bounds__(kBlock) void xt_fill_kernel(const Index* __restrict__ list, Index n, const Index* __restrict__ jptr,
                                                         unsigned int* __restrict__ cursor, Index* __restrict__ jpos) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    const Index c = list[k];
    jpos[jptr[c] + (Index)atomicAdd(&cursor[c], 1u)] = (Index)k;   // (any order: such a result is sorted afterwards)
  }
}

// ---- sizes of the bins, segments of the hub rows, source entries selected: tot[0 .. 3] (row_bins.hpp); row_bin_kernel
// then fills lists that hold exactly what was counted here
__global__ __launch_bounds__(kBlock) void xt_len_kernel(XtRowLen len_of, Index ni, unsigned long long* __restrict__ tot) {
  RowLenSums sums;
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < ni; i += stride) {
    const long long len = len_of(i);
    row_len_add<kXShort, kXSeg>(sums, len);
    sums.n_own += (unsigned long long)len;
  }
  row_len_totals(sums, tot);
}

// One kernel for every bin and pass: groups of G lanes (kXShort or kWave), an item each -- an output row (seg_k ==
// nullptr) or one segment of a hub row.  kMode 0: counts; 1: columns and values; 2: (row, column) keys and value bits.
// jptr == nullptr: J is the identity (every source entry gives itself); jpos == nullptr: a place in J is jptr[c] + q.
template <int G, int kMode>
__global__ __launch_bounds__(kBlock) void xt_rows_kernel(const Index* __restrict__ items, const Index* __restrict__ seg_k, Index nitems,
                                                         const Index* __restrict__ sel, const Index* __restrict__ x_ptr,
                                                         const Index* __restrict__ x_ind, const unsigned int* __restrict__ x_val,
                                                         const Index* __restrict__ jptr, const Index* __restrict__ jpos,
                                                         unsigned int* __restrict__ counts, unsigned int* __restrict__ seg_cnt,
                                                         const Index* __restrict__ c_ptr, const unsigned int* __restrict__ seg_off,
                                                         Index* __restrict__ c_ind, unsigned int* __restrict__ c_val,
                                                         unsigned long long* __restrict__ keys, unsigned int* __restrict__ pay) {
  const int lane = lane_id(), t = lane & (G - 1);
  constexpr int kPerWave = kWave / G;                  // items a wave takes at once
  const long long step = (long long)gridDim.x * kWavesPerBlock * kPerWave;
  // it0 is wave-uniform and every lane stays in the loop: the prefix sums below read across lanes
  for (long long it0 = ((long long)blockIdx.x * kWavesPerBlock + wave_id()) * kPerWave; it0 < nitems; it0 += step) {
    const long long it = it0 + lane / G;
    const bool valid = it < nitems;
    Index i = 0, s = 0, e = 0, k = 0;
    if (valid) {
      i = items[it];
      const Index r = sel ? sel[i] : i;
      s = x_ptr[r];
      e = x_ptr[r + 1];
      if (seg_k) {
        k = seg_k[it];
        s += k * kXSeg;
        e = e < s + kXSeg ? e : s + kXSeg;
      }
    }
    if constexpr (kMode == 0) {
      unsigned long long cnt = 0;
      if (!jptr) {
        cnt = t == 0 ? (unsigned long long)(e - s) : 0ull;
      } else {
        for (Index p = s + t; p < e; p += G) {
          const Index c = x_ind[p];
          cnt += (unsigned long long)(jptr[c + 1] - jptr[c]);
        }
      }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kWave);
      if (valid && t == 0) {
        const unsigned int c32 = cnt >= (unsigned long long)kXSat ? kXSat : (unsigned int)cnt;
        if (seg_k) seg_cnt[it] = c32; else counts[i] = c32;
      }
    } else {
      Index out = 0;
      if (valid) out = seg_k ? c_ptr[i] + (Index)(seg_off[it] - seg_off[it - k]) : c_ptr[i];
      // a short row is one step; the rows of a wave-wide group are the wave's one item, so the bound is wave-uniform
      const Index steps = G == kWave ? (e - s + G - 1) / G : 1;
      for (Index st = 0; st < steps; ++st) {
        const Index p = s + st * G + t;
        Index lo = 0;
        unsigned int n = 0, v = 0;
        if (p < e) {
          const Index c = x_ind[p];
          v = x_val[p];
          if (jptr) { lo = jptr[c]; n = (unsigned int)(jptr[c + 1] - lo); }
          else { lo = c; n = 1; }
        }
        unsigned int incl, total;
        if constexpr (G == kWave) {
          incl = wave_incl_scan_u32(n);
          total = (unsigned int)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        } else {
          incl = row_incl_scan_u32(n);
          total = (unsigned int)__shfl((int)incl, lane | (G - 1), kWave);
        }
        Index pos = out + (Index)(incl - n);
        for (unsigned int q = 0; q < n; ++q, ++pos) {
          const Index col = jpos ? jpos[lo + (Index)q] : lo + (Index)q;
          if constexpr (kMode == 1) {
            c_ind[pos] = col;
            c_val[pos] = v;
          } else {
            keys[pos] = ((unsigned long long)(unsigned int)i << 32) | (unsigned int)col;
            pay[pos] = v;
          }
        }
        out += (Index)total;
      }
    }
  }
}

// a hub row's count: the sum of its segments' (consecutive in the list, in order); one thread per first segment
__global__ __launch_bounds__(kBlock) void xt_fold_kernel(const Index* __restrict__ seg_row, const Index* __restrict__ seg_k, Index nseg,
                                                         const unsigned int* __restrict__ seg_cnt, unsigned int* __restrict__ counts) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long it = (long long)blockIdx.x * kBlock + threadIdx.x; it < nseg; it += stride) {
    if (seg_k[it] != 0) continue;
    const Index i = seg_row[it];
    unsigned int sum = 0;
    for (long long j = it; j < nseg && seg_row[j] == i && seg_k[j] == (Index)(j - it); ++j) sum += seg_cnt[j];
    counts[i] = sum;
  }
}

// sorted (row << 32 | column, value bits) pairs -> columns and values
__global__ __launch_bounds__(kBlock) void xt_unpack_kernel(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ pay,
                                                           Index nnz, Index* __restrict__ c_ind, unsigned int* __restrict__ c_val) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += stride) {
    c_ind[p] = (Index)(unsigned int)keys[p];
    c_val[p] = pay[p];
  }
}

// ---- the vector forms: I[k] probed in one ascending list
__global__ __launch_bounds__(kBlock) void xt_probe_kernel(const Index* __restrict__ sel, Index n, const Index* __restrict__ l_ind,
                                                          Index l_n, unsigned int* __restrict__ flag, Index* __restrict__ at) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    const Index key = sel ? sel[k] : (Index)k;
    Index lo = 0, hi = l_n;
    while (lo < hi) {
      const Index mid = lo + ((hi - lo) >> 1);
      if (l_ind[mid] < key) lo = mid + 1; else hi = mid;
    }
    const bool hit = lo < l_n && l_ind[lo] == key;
    flag[k] = hit ? 1u : 0u;
    at[k] = hit ? lo : -1;
  }
}
// flag: the exclusive scan of the hits
__global__ __launch_bounds__(kBlock) void xt_compact_kernel(Index n, const unsigned int* __restrict__ flag, const Index* __restrict__ at,
                                                            const unsigned int* __restrict__ l_val, Index* __restrict__ w_ind,
                                                            unsigned int* __restrict__ w_val) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    const Index a = at[k];
    if (a < 0) continue;
    w_ind[flag[k]] = (Index)k;
    w_val[flag[k]] = l_val[a];
  }
}
__global__ __launch_bounds__(kBlock) void xt_gather_kernel(const Index* __restrict__ sel, Index n, const unsigned int* __restrict__ u,
                                                           unsigned int* __restrict__ w) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) w[k] = u[sel[k]];
}

// (IndexList: common.hpp -- assign_matrix.hip validates and inverts its lists the same way)
grb_info list_check(IndexList* L, const Index* host, Index n, Index dim) {
  L->host = host;
  L->n = n;
  L->dim = dim;
  if (n < 0) return GRB_DIMENSION_MISMATCH;
  if (!host) return n == dim ? GRB_SUCCESS : GRB_DIMENSION_MISMATCH;
  for (Index k = 0; k < n; ++k) {
    if (host[k] < 0 || host[k] >= dim) return GRB_INDEX_OUT_OF_BOUNDS;
    if (k > 0 && host[k] < host[k - 1]) L->sorted = false;
  }
  return GRB_SUCCESS;
}

grb_info list_upload(IndexList* L) {
  if (!L->host || L->d_list.p) return GRB_SUCCESS;
  GRB_TRY(ewm_alloc(&L->d_list, 4 * (size_t)L->n));
  if (L->n > 0) GRB_HIP_TRY(hipMemcpyAsync(L->d_list.p, L->host, 4 * (size_t)L->n, hipMemcpyHostToDevice, ctx().stream));
  return GRB_SUCCESS;
}

// jptr (and jpos for a list in no order) of a list that is not null
grb_info list_invert(IndexList* L) {
  if (!L->host || L->d_ptr.p) return GRB_SUCCESS;
  hipStream_t s = ctx().stream;
  GRB_TRY(list_upload(L));
  GRB_TRY(ewm_alloc(&L->d_ptr, 4 * ((size_t)L->dim + 1)));
  GRB_HIP_TRY(hipMemsetAsync(L->d_ptr.p, 0, 4 * ((size_t)L->dim + 1), s));
  if (L->n > 0) {
    hipLaunchKernelGGL(xt_hist_kernel, dim3(stream_grid(L->n, kBlock)), dim3(kBlock), 0, s, L->dev(), L->n, (unsigned int*)L->d_ptr.p);
    GRB_HIP_TRY(hipGetLastError());
  }
  EwmBuf scan;
  GRB_TRY(ewm_alloc(&scan, device_scan_u32_scratch((long long)L->dim + 1)));
  GRB_TRY(device_exclusive_scan_u32_in((unsigned int*)L->d_ptr.p, (long long)L->dim + 1, (unsigned int*)scan.p));
  if (L->sorted) return GRB_SUCCESS;
  EwmBuf cursor;
  GRB_TRY(ewm_alloc(&cursor, 4 * (size_t)L->dim));
  GRB_TRY(ewm_alloc(&L->d_pos, 4 * (size_t)L->n));
  GRB_HIP_TRY(hipMemsetAsync(cursor.p, 0, 4 * (size_t)L->dim, s));
  hipLaunchKernelGGL(xt_fill_kernel, dim3(stream_grid(L->n, kBlock)), dim3(kBlock), 0, s, L->dev(), L->n, L->jptr(),
                     (unsigned int*)cursor.p, (Index*)L->d_pos.p);
  GRB_HIP_TRY(hipGetLastError());
  GRB_HIP_TRY(hipStreamSynchronize(s));                  // (the cursors are freed on the way out)
  return GRB_SUCCESS;
}

namespace {

template <int kMode>
grb_info launch_rows(hipStream_t s, const RowBins& b, const Index* sel, const CsrArrays& X, const Index* jptr, const Index* jpos,
                     unsigned int* counts, const Index* c_ptr, Index* c_ind, unsigned int* c_val, unsigned long long* keys,
                     unsigned int* pay) {
  return for_each_bin<kXShort>(b, [&](auto g, int grid, const Index* items, const Index* seg_k, Index n) {
    unsigned int* seg_cnt = seg_k ? b.seg_cnt : nullptr;   // a segment's count (kMode 0), then its offset
    hipLaunchKernelGGL((xt_rows_kernel<decltype(g)::value, kMode>), dim3(grid), dim3(kBlock), 0, s, items, seg_k, n, sel, X.ptr, X.ind,
                       (const unsigned int*)X.val, jptr, jpos, counts, seg_cnt, c_ptr, seg_cnt, c_ind, c_val, keys, pay);
  });
}

// one orientation: out = X(R, Cl), X's rows selected by R, its columns by Cl
grb_info extract_side(const CsrArrays& X, IndexList* R, IndexList* Cl, Side* out) {
  hipStream_t s = ctx().stream;
  const Index ni = R->n;
  GRB_TRY(list_upload(R));
  GRB_TRY(list_invert(Cl));
  const Index* sel = R->dev();
  const XtRowLen len_of{sel, X.ptr};
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)ni + 1)));
  unsigned int* counts = (unsigned int*)out->ptr.p;
  GRB_HIP_TRY(hipMemsetAsync(counts, 0, 4 * ((size_t)ni + 1), s));
  // an output row appears once per occurrence in I, so nothing bounds the bins beforehand: a length pass sizes them
  RowBins b;
  GRB_TRY(row_bins_head(&b, s));
  if (ni > 0) {
    hipLaunchKernelGGL(xt_len_kernel, dim3(stream_grid(ni, kBlock * 8)), dim3(kBlock), 0, s, len_of, ni, b.d_tot);
    GRB_HIP_TRY(hipGetLastError());
  }
  GRB_TRY(row_bins_sized(&b, ni, s));
  // every column selected once (a null list): the result has the selected source entries, known already
  if (!Cl->host && b.own > (unsigned long long)INT32_MAX) return GRB_OUT_OF_MEMORY;
  if (ni > 0) GRB_TRY((row_bins_fill<kXShort, kXSeg>(b, len_of, ni, s)));
  // ---- symbolic
  GRB_TRY(launch_rows<0>(s, b, sel, X, Cl->jptr(), nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr));
  GRB_TRY(row_bins_total(b, counts, ni, true, s, out));  // (a hub row's own count is still zero here)
  if (b.nbin[2]) {
    hipLaunchKernelGGL(xt_fold_kernel, dim3(stream_grid((long long)b.nbin[2], kBlock)), dim3(kBlock), 0, s, b.seg_row, b.seg_k,
                       (Index)b.nbin[2], b.seg_cnt, counts);
    GRB_HIP_TRY(hipGetLastError());
  }
  GRB_TRY(row_bins_pointers(b, ni, out, false));
  // ---- numeric
  if (Cl->sorted) {
    GRB_TRY(side_alloc_entries(out));
    if (out->nnz == 0) return GRB_SUCCESS;
    GRB_TRY(launch_rows<1>(s, b, sel, X, Cl->jptr(), nullptr, nullptr, (const Index*)counts, (Index*)out->ind.p,
                           (unsigned int*)out->val.p, nullptr, nullptr));
    GRB_HIP_TRY(hipStreamSynchronize(s));                // (the lists are freed on the way out)
    return GRB_SUCCESS;
  }
  // J in no order: (row, column) keys, sorted over the bits the two dimensions need
  const size_t cap = (size_t)(out->nnz > 0 ? out->nnz : 1);
  EwmBuf pairs;
  if (out->nnz > 0) {
    GRB_TRY(ewm_alloc(&pairs, 12 * cap));
    unsigned long long* keys = (unsigned long long*)pairs.p;
    unsigned int* pay = (unsigned int*)(keys + cap);
    GRB_TRY(launch_rows<2>(s, b, sel, X, Cl->jptr(), Cl->jpos(), nullptr, (const Index*)counts, nullptr, nullptr, keys, pay));
    GRB_TRY(device_sort_pairs(keys, pay, out->nnz, index_bits(Cl->n), index_bits(ni)));
  }
  GRB_TRY(side_alloc_entries(out));
  if (out->nnz > 0) {
    hipLaunchKernelGGL(xt_unpack_kernel, dim3(stream_grid(out->nnz, kBlock)), dim3(kBlock), 0, s, (const unsigned long long*)pairs.p,
                       (const unsigned int*)((const unsigned long long*)pairs.p + cap), out->nnz, (Index*)out->ind.p,
                       (unsigned int*)out->val.p);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipStreamSynchronize(s));                // (the pairs are freed on the way out)
  }
  return GRB_SUCCESS;
}


// w <- the entries k where sel[k] (k itself for a null list) is in the ascending list (l_ind, l_val); w becomes sparse
grb_info probe_into(grb_vector w, const IndexList& L, const Index* l_ind, const void* l_val, Index l_n) {
  hipStream_t s = ctx().stream;
  const Index n = L.n;
  EwmBuf flag, at, o_ind, o_val, scan;
  GRB_TRY(ewm_alloc(&flag, 4 * ((size_t)n + 1)));
  GRB_TRY(ewm_alloc(&at, 4 * (size_t)n));
  GRB_TRY(ewm_alloc(&o_ind, 4 * (size_t)n));
  GRB_TRY(ewm_alloc(&o_val, 4 * (size_t)n));
  GRB_TRY(ewm_alloc(&scan, device_scan_u32_scratch((long long)n + 1)));
  GRB_HIP_TRY(hipMemsetAsync(flag.p, 0, 4 * ((size_t)n + 1), s));
  unsigned int hits = 0;
  if (n > 0) {
    hipLaunchKernelGGL(xt_probe_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, L.dev(), n, l_ind, l_n, (unsigned int*)flag.p,
                       (Index*)at.p);
    GRB_HIP_TRY(hipGetLastError());
    GRB_TRY(device_exclusive_scan_u32_in((unsigned int*)flag.p, (long long)n + 1, (unsigned int*)scan.p));
    hipLaunchKernelGGL(xt_compact_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, n, (const unsigned int*)flag.p,
                       (const Index*)at.p, (const unsigned int*)l_val, (Index*)o_ind.p, (unsigned int*)o_val.p);
    GRB_HIP_TRY(hipGetLastError());
    GRB_HIP_TRY(hipMemcpyAsync(&hits, (unsigned int*)flag.p + n, 4, hipMemcpyDeviceToHost, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  // everything that can fail is behind us (w may be the list's owner: its storage is written only now)
  GRB_TRY(grb_vector_set_storage(w, GRB_SPARSE));
  if (hits > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(w->s_ind, o_ind.p, 4 * (size_t)hits, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemcpyAsync(w->s_val, o_val.p, 4 * (size_t)hits, hipMemcpyDeviceToDevice, s));
  }
  GRB_HIP_TRY(hipStreamSynchronize(s));
  w->s_nvals = (Index)hits;
  w->nvals = (Index)hits;
  return GRB_SUCCESS;
}

}  // namespace

grb_info extract_matrix(grb_matrix C, grb_matrix A, const Index* rows, Index nrows, const Index* cols, Index ncols, bool tran) {
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  if (nrows != C->nrows || ncols != C->ncols) return GRB_DIMENSION_MISMATCH;
  const Index m = tran ? A->ncols : A->nrows, n = tran ? A->nrows : A->ncols;   // op(A) is m x n
  IndexList I, J;
  GRB_TRY(list_check(&I, rows, nrows, m));
  GRB_TRY(list_check(&J, cols, ncols, n));
  if ((tran && !has_csc(A)) || !A->csr.ptr) return GRB_INVALID_OBJECT;
  const CsrArrays& Xr = tran ? A->csc : A->csr;          // rows of op(A)
  const CsrArrays& Xc = tran ? A->csr : A->csc;          // its columns
  const bool both = C->format != 1 && (tran || has_csc(A));
  Side r, c;
  GRB_TRY(extract_side(Xr, &I, &J, &r));
  if (both) GRB_TRY(extract_side(Xc, &J, &I, &c));
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));       // (the lists are the caller's; A may be C)
  return attach(C, &r, both ? &c : nullptr);
}

grb_info extract_matrix_col(grb_vector w, grb_matrix A, const Index* rows, Index nrows, Index col, bool tran) {
  if ((A->dtype != GRB_F32 && A->dtype != GRB_I32) || w->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  if (nrows != w->nsize) return GRB_DIMENSION_MISMATCH;
  const Index m = tran ? A->ncols : A->nrows, n = tran ? A->nrows : A->ncols;   // op(A) is m x n
  IndexList I;
  GRB_TRY(list_check(&I, rows, nrows, m));
  if (col < 0 || col >= n) return GRB_INDEX_OUT_OF_BOUNDS;
  if ((!tran && !has_csc(A)) || !A->csr.ptr) return GRB_INVALID_OBJECT;
  const CsrArrays& X = tran ? A->csr : A->csc;           // column j of op(A) is row j of this orientation
  const std::vector<Index>& hp = tran ? A->h_csr_ptr : A->h_csc_ptr;
  Index lo = 0, hi = 0;
  if (hp.size() == (size_t)n + 1) { lo = hp[(size_t)col]; hi = hp[(size_t)col + 1]; }
  else {
    Index two[2];
    GRB_HIP_TRY(hipMemcpyAsync(two, X.ptr + col, 8, hipMemcpyDeviceToHost, ctx().stream));
    GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
    lo = two[0]; hi = two[1];
  }
  GRB_TRY(list_upload(&I));
  return probe_into(w, I, X.ind + lo, (const char*)X.val + 4 * (size_t)lo, hi - lo);
}

grb_info extract_vector(grb_vector w, grb_vector u, const Index* indices, Index nindices) {
  if (u->vec_type != GRB_SPARSE && u->vec_type != GRB_DENSE) return GRB_UNINITIALIZED_OBJECT;
  if (w->dtype != u->dtype) return GRB_DOMAIN_MISMATCH;
  if (nindices != w->nsize) return GRB_DIMENSION_MISMATCH;
  IndexList I;
  GRB_TRY(list_check(&I, indices, nindices, u->nsize));
  GRB_TRY(list_upload(&I));
  if (u->vec_type == GRB_SPARSE) return probe_into(w, I, u->s_ind, u->s_val, u->s_nvals);
  hipStream_t s = ctx().stream;
  const Index n = nindices;
  EwmBuf tmp;                                            // (w may be u)
  GRB_TRY(ewm_alloc(&tmp, 4 * (size_t)n));
  if (n > 0 && I.host) {
    hipLaunchKernelGGL(xt_gather_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, I.dev(), n, (const unsigned int*)u->d_val,
                       (unsigned int*)tmp.p);
    GRB_HIP_TRY(hipGetLastError());
  }
  GRB_TRY(grb_vector_set_storage(w, GRB_DENSE));
  if (n > 0 && (I.host || w != u))
    GRB_HIP_TRY(hipMemcpyAsync(w->d_val, I.host ? tmp.p : u->d_val, 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
  GRB_HIP_TRY(hipStreamSynchronize(s));
  w->d_nnz = n;
  return GRB_SUCCESS;
}

}  // namespace grb

using namespace grb;

// extract (operations.hpp:355-410): the contract is the comment in include/grb_hip.h
grb_info grb_matrix_extract(grb_matrix C, grb_matrix mask, grb_accum accum, grb_matrix A, const grb_index* row_indices,
                            grb_index nrows, const grb_index* col_indices, grb_index ncols, grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  if (!C || !A) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built || (mask && !mask->built)) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return extract_matrix(C, A, row_indices, nrows, col_indices, ncols, desc && desc->desc[GRB_INP0] == GRB_TRAN);
}

grb_info grb_matrix_extract_col(grb_vector w, grb_vector mask, grb_accum accum, grb_matrix A, const grb_index* row_indices,
                                grb_index nrows, grb_index col_index, grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  if (!w || !A) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return extract_matrix_col(w, A, row_indices, nrows, col_index, desc && desc->desc[GRB_INP0] == GRB_TRAN);
}

grb_info grb_vector_extract(grb_vector w, grb_vector mask, grb_accum accum, grb_vector u, const grb_index* indices,
                            grb_index nindices, grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  (void)desc;
  if (!w || !u) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return extract_vector(w, u, indices, nindices);
}
