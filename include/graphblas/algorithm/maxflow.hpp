// graphblas/algorithm/maxflow.hpp -- maximum flow and minimum cut through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// function goes straight to the library's grb_maxflow, whose contract is the comment in grb_hip.h.
//   maxflow(F, side, A, source, sink, mode, desc)   the maximum flow from source to sink over the arcs A(i, j) = the capacity of
//                                                   i -> j; F = a maximum flow in cancelled form, side(v) = 1 when sink can
//                                                   be reached from v in the residual graph (the smallest sink side of a
//                                                   minimum cut)
// mode: GRB_FLOW_CAPACITY (0, the values are the capacities: int >= 0, float an integer value in 0 .. 2^24, anything else is
// GrB_INVALID_VALUE) or GRB_FLOW_UNIT (1, every stored off-diagonal entry has capacity 1; the values are not read).  A: n x n,
// float or int, directed, with columns of its own (GrB_INVALID_OBJECT otherwise); its diagonal takes no part.  F: NULL, or
// n x n of A's type; F may be A.  side: NULL, or an int vector of size n, dense afterwards.  desc may be NULL (no field is
// read).  Returns the Info of the call; the optional last argument receives the library's record (the value, the arcs, the
// flow's and the cut's sizes, the cut's capacity, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_MAXFLOW_HPP_
#define GRB_HIP_ALGORITHM_MAXFLOW_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info maxflow(Matrix<T>* F, Vector<int>* side, const Matrix<T>* A, Index source, Index sink, int mode, Descriptor* desc,
                    grb_maxflow_result* result = NULL) {
  if (A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_maxflow(F ? F->handle() : static_cast<grb_matrix>(NULL), side ? side->handle() : static_cast<grb_vector>(NULL),
                             A->handle(), static_cast<int64_t>(source), static_cast<int64_t>(sink), mode,
                             desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A (the template argument is deduced from F and A alike)
template <typename T>
inline Info maxflow(Matrix<T>* F, Vector<int>* side, Matrix<T>* A, Index source, Index sink, int mode, Descriptor* desc,
                    grb_maxflow_result* result = NULL) {
  return maxflow<T>(F, side, static_cast<const Matrix<T>*>(A), source, sink, mode, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_MAXFLOW_HPP_
