// kronecker.hip -- GraphBLAS's Kronecker product (GrB_kronecker; the reference declares no such operation):
// grb_kronecker, C = op(A) (x) op(B).  The contract is the comment in include/grb_hip.h.
//
// One orientation of op(A) (mA rows) against one of op(B) (mB rows, nB columns) is a closed form: nothing is counted,
// scanned or sorted.  Row r = iA * mB + iB of C holds lenA(iA) * lenB(iB) entries and begins at
//   ptrC[r] = ptrA[iA] * nnzB + lenA(iA) * ptrB[iB]
// (the rows of one iA are a block of lenA(iA) * nnzB entries), and entry t of it, a = t / lenB(iB), b = t % lenB(iB), is
//   column indA[ptrA[iA] + a] * nB + indB[ptrB[iB] + b],  value mul(valA[ptrA[iA] + a], valB[ptrB[iB] + b]).
// Columns ascend because both inputs' do.  The kernel is bound by the stores of C (8 bytes an entry against the two cached
// gathers that make it), so the work is cut over C's entries, whatever its rows look like:
//   tiles     the positions [0, nnzC) in tiles of kKronTile = 2048: a workgroup per tile, a wave per 512 consecutive
//             positions, a lane per four consecutive positions in each of two steps -- every store is 16 bytes a lane, a
//             wave's is 1 KiB of consecutive words of indC and of valC.
//   rows      position p lies in the block of the row of A that holds A's entry p / nnzB, and, q into that block, in the
//             row of B that holds B's entry q / lenA: two searches of a pointer array for the row of an entry.  A wave
//             finds the rows of its first and its last position with the whole wave probing (64 places a round); a lane
//             then bisects between those two answers only.  Inside one row of C -- a hub row of A against a hub row of B
//             spans many tiles -- the two answers are equal and no lane searches at all; a run of thousands of empty rows
//             (an empty row of A is mB empty rows of C) is a dozen probes, never a walk over the rows.
//   walk      a lane locates its first position and steps b, then a, through the other three; only a position that
//             begins a new row of C is located again.
// C's other orientation is the same routine over the other orientations of op(A) and op(B): (A (x) B)^T = A^T (x) B^T,
// with mul still taking A's value first.  The row pointers are a launch of their own, a thread per row.
#include "common.hpp"

namespace grb {

constexpr int kKronVec = 4;                                          // consecutive positions of one lane: one 16-byte store
constexpr int kKronSteps = 2;                                        // steps of kWave * kKronVec positions per wave
constexpr int kKronWaveTile = kWave * kKronVec * kKronSteps;         // consecutive positions of one wave
constexpr int kKronTile = kKronWaveTile * kWavesPerBlock;            // ... of one workgroup

// the largest r with ptr[r] <= x, for 0 <= x < ptr[nrows]: the row of entry x.  The whole wave probes, 64 places a round
// (select.hip: sel_find_row).
__device__ inline Index kron_find_row(const Index* __restrict__ ptr, Index nrows, unsigned int x, int lane) {
  long long lo = 0, hi = nrows;                          // ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const long long step = (hi - lo + kWave - 1) / kWave;
    const long long q = lo + (lane + 1) * step;
    const bool le = q < hi && (unsigned int)ptr[q] <= x;
    lo += __popcll(__ballot(le)) * step;                 // (ptr ascends: the probes that pass are the first ones)
    hi = lo + step < hi ? lo + step : hi;
  }
  return (Index)lo;
}

// the same answer by one lane, known to lie in [lo, hi]
__device__ __forceinline__ Index kron_lane_row(const Index* __restrict__ ptr, Index lo, Index hi, unsigned int x) {
  while (lo < hi) {
    const Index mid = lo + (hi - lo + 1) / 2;
    if ((unsigned int)ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// MUL: a BinOp, or -1 for the multiply of the registered semiring in constant memory
template <int MUL, typename T>
__device__ __forceinline__ T kron_mul(T a, T b) {
  if constexpr (MUL < 0) return binop_rt<T>(rt_semiring().mul_op, a, b);
  else return binop<MUL, T>(a, b);
}

// ptrC[r] for r in [0, mC]; 64-bit products (the host has checked that the last one, nnzC, fits an Index)
__global__ __launch_bounds__(kBlock) void kron_ptr_kernel(const Index* __restrict__ ptrA, const Index* __restrict__ ptrB, Index mB,
                                                          long long nnzB, long long mC, Index nnz, Index* __restrict__ ptrC) {
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r <= mC; r += (long long)gridDim.x * kBlock) {
    if (r == mC) {
      ptrC[r] = nnz;
      continue;
    }
    const long long iA = r / mB, iB = r - iA * mB;
    const long long pa = ptrA[iA], la = ptrA[iA + 1] - pa;
    ptrC[r] = (Index)(pa * nnzB + la * ptrB[iB]);
  }
}

// The entries of C, positions [0, nnz): nnz = nnzA * nnzB <= INT32_MAX, so every position, every offset into a block and
// every row length below fits 32 bits; a column indA * nB + indB is below C's width, an Index.  One workgroup per tile.
template <int MUL, typename T>
__global__ __launch_bounds__(kBlock) void kron_kernel(const Index* __restrict__ ptrA, Index mA, const Index* __restrict__ indA,
                                                      const T* __restrict__ valA, const Index* __restrict__ ptrB, Index mB,
                                                      const Index* __restrict__ indB, const T* __restrict__ valB, unsigned int nnzB,
                                                      unsigned int nB, unsigned int nnz, Index* __restrict__ indC,
                                                      unsigned int* __restrict__ valC) {
  const int lane = lane_id();
  const unsigned int w0 = blockIdx.x * (unsigned int)kKronTile + (unsigned int)wave_id() * kKronWaveTile;
  if (w0 >= nnz) return;                                 // (wave-uniform; no workgroup barrier below)
  const unsigned int w1 = nnz - w0 > (unsigned int)kKronWaveTile ? w0 + kKronWaveTile : nnz;   // the wave's positions: [w0, w1)
  // the rows of A and of B of the wave's first and last position: every lane's rows lie between them
  const unsigned int x0 = w0 / nnzB, x1 = (w1 - 1) / nnzB;
  const Index a_lo = kron_find_row(ptrA, mA, x0, lane);
  const Index a_hi = x1 == x0 ? a_lo : kron_find_row(ptrA, mA, x1, lane);
  Index b_lo = 0, b_hi = mB - 1;
  if (a_lo == a_hi) {                                    // one block: the rows of B narrow too
    const unsigned int pa = (unsigned int)ptrA[a_lo], la = (unsigned int)ptrA[a_lo + 1] - pa;
    const unsigned int y0 = (w0 - pa * nnzB) / la, y1 = (w1 - 1 - pa * nnzB) / la;
    b_lo = kron_find_row(ptrB, mB, y0, lane);
    b_hi = y1 == y0 ? b_lo : kron_find_row(ptrB, mB, y1, lane);
  }
#pragma unroll
  for (int k = 0; k < kKronSteps; ++k) {
    const unsigned int p = w0 + (unsigned int)(k * kWave * kKronVec + lane * kKronVec);
    if (p >= w1) continue;
    unsigned int left = 0;                               // entries of the current row of C from the current position on
    unsigned int eA = 0, eB = 0, b = 0, lenB = 1, colA = 0;
    T va = T();
    unsigned int cols[kKronVec], vals[kKronVec];
#pragma unroll
    for (int j = 0; j < kKronVec; ++j) {
      cols[j] = 0u;
      vals[j] = 0u;
      if (p + j < w1) {
        if (left == 0) {                                 // locate position p + j
          const unsigned int pj = p + j;
          const Index iA = kron_lane_row(ptrA, a_lo, a_hi, pj / nnzB);
          const unsigned int pa = (unsigned int)ptrA[iA], la = (unsigned int)ptrA[iA + 1] - pa;   // la > 0: the row holds an entry
          const unsigned int q = pj - pa * nnzB;
          const Index iB = kron_lane_row(ptrB, b_lo, b_hi, q / la);
          eB = (unsigned int)ptrB[iB];
          lenB = (unsigned int)ptrB[iB + 1] - eB;        // > 0 likewise
          const unsigned int t = q - la * eB;
          const unsigned int a = t / lenB;
          b = t - a * lenB;
          eA = pa + a;
          left = la * lenB - t;
          colA = (unsigned int)indA[eA] * nB;
          va = valA[eA];
        }
        cols[j] = colA + (unsigned int)indB[eB + b];
        const T v = kron_mul<MUL, T>(va, valB[eB + b]);
        memcpy(&vals[j], &v, 4);
        --left;
        if (++b == lenB) {
          b = 0;
          ++eA;
          if (left) {                                    // (the row's last entry has no successor to read)
            colA = (unsigned int)indA[eA] * nB;
            va = valA[eA];
          }
        }
      }
    }
    if (p + kKronVec <= w1) {                            // p is a multiple of four and the arrays are allocations: aligned
      *reinterpret_cast<uint4*>(indC + p) = make_uint4(cols[0], cols[1], cols[2], cols[3]);
      *reinterpret_cast<uint4*>(valC + p) = make_uint4(vals[0], vals[1], vals[2], vals[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kKronVec; ++j)
        if (p + j < w1) {
          indC[p + j] = (Index)cols[j];
          valC[p + j] = vals[j];
        }
    }
  }
}

namespace {

// one orientation: the mX rows of X against the mY rows (nY columns) of Y -> out, mX * mY rows of nnz entries.  The launches
// and the copy of the pointers are left in flight: the caller synchronises the stream.
grb_info kron_side(int op, int dtype, const CsrArrays& X, Index mX, Index nnzX, const CsrArrays& Y, Index mY, Index nY, Index nnzY,
                   Side* out) {
  hipStream_t s = ctx().stream;
  const long long mC = (long long)mX * mY;
  const Index nnz = (Index)((long long)nnzX * nnzY);
  out->nnz = nnz;
  GRB_TRY(ewm_alloc(&out->ptr, 4 * ((size_t)mC + 1)));
  GRB_TRY(ewm_alloc(&out->ind, 4 * (size_t)(nnz > 0 ? nnz : 1)));
  GRB_TRY(ewm_alloc(&out->val, 4 * (size_t)(nnz > 0 ? nnz : 1)));
  Index* ptrC = (Index*)out->ptr.p;
  if (nnz == 0) {
    GRB_HIP_TRY(hipMemsetAsync(ptrC, 0, 4 * ((size_t)mC + 1), s));
  } else {
    hipLaunchKernelGGL(kron_ptr_kernel, dim3(stream_grid(mC + 1)), dim3(kBlock), 0, s, X.ptr, Y.ptr, mY, (long long)nnzY, mC, nnz, ptrC);
    GRB_HIP_TRY(hipGetLastError());
    const int ntiles = (int)(((long long)nnz + kKronTile - 1) / kKronTile);
    GRB_TRY(dispatch_semiring(op, dtype, [&](auto tag, auto tv) -> grb_info {
      using T = decltype(tv);
      constexpr int MUL = Semiring<decltype(tag)::value, T>::mulop;
      hipLaunchKernelGGL((kron_kernel<MUL, T>), dim3(ntiles), dim3(kBlock), 0, s, X.ptr, mX, X.ind, (const T*)X.val, Y.ptr, mY, Y.ind,
                         (const T*)Y.val, (unsigned int)nnzY, (unsigned int)nY, (unsigned int)nnz, (Index*)out->ind.p,
                         (unsigned int*)out->val.p);
      GRB_HIP_TRY(hipGetLastError());
      return GRB_SUCCESS;
    }));
  }
  out->h_ptr.resize((size_t)mC + 1);
  GRB_HIP_TRY(hipMemcpyAsync(out->h_ptr.data(), ptrC, 4 * ((size_t)mC + 1), hipMemcpyDeviceToHost, s));
  return GRB_SUCCESS;
}

}  // namespace

grb_info kronecker_matrix(grb_matrix C, int op, grb_matrix A, grb_matrix B, bool tran_a, bool tran_b) {
  if (!(A->dtype == GRB_F32 || A->dtype == GRB_I32) || B->dtype != A->dtype || C->dtype != A->dtype) return GRB_NOT_IMPLEMENTED;
  const Index mA = tran_a ? A->ncols : A->nrows, nA = tran_a ? A->nrows : A->ncols;   // op(A) is mA x nA
  const Index mB = tran_b ? B->ncols : B->nrows, nB = tran_b ? B->nrows : B->ncols;
  if ((long long)C->nrows != (long long)mA * mB || (long long)C->ncols != (long long)nA * nB) return GRB_DIMENSION_MISMATCH;
  if ((tran_a && !has_csc(A)) || (tran_b && !has_csc(B)) || !A->csr.ptr || !B->csr.ptr) return GRB_INVALID_OBJECT;
  if (op >= GRB_USER_SEMIRING_BASE) {
    UserSemiring u;
    if (!user_semiring_lookup(op, &u)) return GRB_INVALID_VALUE;
  } else if (op < 0 || op >= GRB_N_SEMIRINGS) {
    return GRB_INVALID_VALUE;
  }
  if ((long long)A->nvals * (long long)B->nvals > (long long)INT32_MAX) return GRB_OUT_OF_MEMORY;   // grb_index is 32 bits
  const CsrArrays& Ar = tran_a ? A->csc : A->csr;        // rows of op(A)
  const CsrArrays& Br = tran_b ? B->csc : B->csr;
  const CsrArrays& Ac = tran_a ? A->csr : A->csc;        // its columns
  const CsrArrays& Bc = tran_b ? B->csr : B->csc;
  // C's CSC: the same routine over the other orientations, when both inputs have theirs (and C is not CSR only)
  const bool both = C->format != 1 && (tran_a || has_csc(A)) && (tran_b || has_csc(B));
  Side r, c;
  GRB_TRY(kron_side(op, A->dtype, Ar, mA, A->nvals, Br, mB, nB, B->nvals, &r));
  if (both) GRB_TRY(kron_side(op, A->dtype, Ac, nA, A->nvals, Bc, nB, mB, B->nvals, &c));
  GRB_HIP_TRY(hipStreamSynchronize(ctx().stream));
  return attach(C, &r, both ? &c : nullptr);             // (A or B may be C: both sides have synchronised)
}

}  // namespace grb

using namespace grb;

// kronecker: the contract is the comment in include/grb_hip.h
grb_info grb_kronecker(grb_matrix C, grb_matrix mask, grb_accum accum, grb_semiring op, grb_matrix A, grb_matrix B,
                       grb_descriptor desc) { GRB_API_ENTER();
  (void)accum;
  if (!C || !A || !B) return GRB_UNINITIALIZED_OBJECT;
  if (!A->built || !B->built || (mask && !mask->built)) return GRB_UNINITIALIZED_OBJECT;
  if (mask) return GRB_NOT_IMPLEMENTED;
  return kronecker_matrix(C, (int)op, A, B, desc && desc->desc[GRB_INP0] == GRB_TRAN, desc && desc->desc[GRB_INP1] == GRB_TRAN);
}
