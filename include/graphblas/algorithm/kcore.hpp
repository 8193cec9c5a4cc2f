// graphblas/algorithm/kcore.hpp -- the k-core decomposition through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// functions go straight to the library's grb_coreness and grb_kcore, whose contract is the comment in grb_hip.h.
//   coreness(core, A, desc)   core(v) = the largest k such that v is in the k-core, the largest subgraph in which every
//                             vertex has at least k neighbours inside the subgraph; 0 for an isolated vertex
//   kcore(v, A, k, desc)      v(x) = the number of x's neighbours inside the k-core when x is in it (>= k), else 0
// A: n x n, float or int, with the same structure as its transpose (checked when A has columns of its own:
// GrB_INVALID_VALUE otherwise); its values are never read and its diagonal takes no part.  core / v: an int vector of size
// n, dense afterwards.  desc may be NULL (no field is read).  k < 0 is GrB_INVALID_VALUE.  Returns the Info of the call; the
// optional last argument receives the library's record (edges, the edges and vertices of the kmax-core or of the k-core,
// kmax, the distinct core numbers, the device's passes and launches, the time of the device work).
#ifndef GRB_HIP_ALGORITHM_KCORE_HPP_
#define GRB_HIP_ALGORITHM_KCORE_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename a>
inline Info coreness(Vector<int>* core, const Matrix<a>* A, Descriptor* desc, grb_kcore_result* result = NULL) {
  if (core == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_coreness(core->handle(), A->handle(), desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

template <typename a>
inline Info kcore(Vector<int>* v, const Matrix<a>* A, int k, Descriptor* desc, grb_kcore_result* result = NULL) {
  if (v == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_kcore(v->handle(), A->handle(), k, desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_KCORE_HPP_
