// graphblas/algorithm/bc.hpp -- betweenness centrality through the drop-in frontend.  The reference has no such driver
// (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the function
// goes straight to the library's grb_bc, whose contract is the comment in grb_hip.h.
//   bc(v, A, sources, desc)   v(x) = the sum over the sources s of delta_s(x): batched Brandes, 64 sources per sweep
// A: n x n, float or int; its values are never read, a stored A(i, j) is the edge i -> j, its diagonal takes no part and
// its structure need not be symmetric.  sources: vertex ids, or NULL for every vertex (exact centrality).  v: a float
// vector of size n, dense afterwards; not normalised, not halved.  desc may be NULL (no field is read).  Returns the Info
// of the call; the optional last argument receives the library's record (sources, batches, levels, vertices reached, the
// time of the loop).
#ifndef GRB_HIP_ALGORITHM_BC_HPP_
#define GRB_HIP_ALGORITHM_BC_HPP_

#include <vector>

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename a>
inline Info bc(Vector<float>* v, const Matrix<a>* A, const std::vector<Index>* sources, Descriptor* desc,
               grb_bc_result* result = NULL) {
  if (v == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  static const grb_index none = 0;                       // an empty list is an error of the call, not "every vertex"
  const grb_index* list = !sources ? static_cast<const grb_index*>(NULL) : sources->empty() ? &none : sources->data();
  const int ns = sources ? static_cast<int>(sources->size()) : 0;
  return to_info(grb_bc(v->handle(), A->handle(), list, ns, desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_BC_HPP_
