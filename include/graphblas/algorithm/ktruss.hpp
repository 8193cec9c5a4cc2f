// graphblas/algorithm/ktruss.hpp -- k-truss and edge trussness through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// two functions go straight to the library's grb_ktruss / grb_trussness, whose contract is the comment in grb_hip.h.
//   ktruss(C, A, k, desc)     C = the k-truss of A's graph; C(i, j) = the support of the edge {i, j} in it
//   trussness(C, A, desc)     C = A's graph; C(i, j) = the largest k such that {i, j} is in the k-truss
// A: n x n, symmetric in structure; its values are never read and its diagonal takes no part.  C: n x n, float or int
// whatever A's type, both orientations; C may be A.  desc may be NULL (no field is read).  Both return the Info of the
// call; the optional last argument receives the library's record (rounds, support computations, edges, kmax, the time of
// the loop).
#ifndef GRB_HIP_ALGORITHM_KTRUSS_HPP_
#define GRB_HIP_ALGORITHM_KTRUSS_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename c, typename a>
inline Info ktruss(Matrix<c>* C, const Matrix<a>* A, int k, Descriptor* desc, grb_truss_result* result = NULL) {
  if (C == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  const Info i = to_info(grb_ktruss(C->handle(), A->handle(), k, desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
  if (i != GrB_SUCCESS) return i;
  return C->refresh_all();
}

template <typename c, typename a>
inline Info trussness(Matrix<c>* C, const Matrix<a>* A, Descriptor* desc, grb_truss_result* result = NULL) {
  if (C == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  const Info i = to_info(grb_trussness(C->handle(), A->handle(), desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
  if (i != GrB_SUCCESS) return i;
  return C->refresh_all();
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_KTRUSS_HPP_
