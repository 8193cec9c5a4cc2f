// graphblas/algorithm/scc.hpp -- the strongly connected components through the drop-in frontend.  The reference has no
// such driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers:
// the function goes straight to the library's grb_scc, whose contract is the comment in grb_hip.h.
//   scc(v, A, desc)   v(x) = the smallest vertex number in x's strongly connected component: the vertices that reach x and
//                     are reached from x along A's off-diagonal entries
// A: n x n, float or int, with a CSC of its own (GrB_INVALID_OBJECT for a product result or the CSR-only format); its values
// are never read and its diagonal takes no part.  v: an int vector of size n, dense afterwards.  desc may be NULL (no field
// is read: the transpose has the same components).  Returns the Info of the call; the optional last argument receives the
// library's record (edges, the components, the largest one, the single vertices, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_SCC_HPP_
#define GRB_HIP_ALGORITHM_SCC_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename a>
inline Info scc(Vector<int>* v, const Matrix<a>* A, Descriptor* desc, grb_scc_result* result = NULL) {
  if (v == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_scc(v->handle(), A->handle(), desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_SCC_HPP_
