// graphblas/algorithm/msf.hpp -- the minimum spanning forest through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// function goes straight to the library's grb_msf, whose contract is the comment in grb_hip.h.
//   msf(C, comp, A, desc)   C = the minimum spanning forest of A's weighted undirected graph under the total order of the
//                           keys (w, min(u, v), max(u, v)): both directions of every forest edge with A's weight;
//                           comp(v) = the smallest vertex number in v's connected component
// A: n x n, float or int, symmetric in structure and in values (checked when A has columns of its own: GrB_INVALID_VALUE
// otherwise, as is a NaN off the diagonal); its diagonal takes no part.  C: n x n of A's type; C may be A.  comp: an int
// vector of size n, dense afterwards, or NULL.  desc may be NULL (no field is read).  Returns the Info of the call; the
// optional last argument receives the library's record (edges, the forest's edges and weight, the components, the isolated
// vertices, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_MSF_HPP_
#define GRB_HIP_ALGORITHM_MSF_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info msf(Matrix<T>* C, Vector<int>* comp, const Matrix<T>* A, Descriptor* desc, grb_msf_result* result = NULL) {
  if (C == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_msf(C->handle(), comp ? comp->handle() : static_cast<grb_vector>(NULL), A->handle(),
                         desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A (the template argument is deduced from C and A alike)
template <typename T>
inline Info msf(Matrix<T>* C, Vector<int>* comp, Matrix<T>* A, Descriptor* desc, grb_msf_result* result = NULL) {
  return msf<T>(C, comp, static_cast<const Matrix<T>*>(A), desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_MSF_HPP_
