// graphblas/algorithm/lcc.hpp -- the local clustering coefficient through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// function goes straight to the library's grb_lcc, whose contract is the comment in grb_hip.h.
//   lcc(lcc, A, directed, desc)   lcc(v) = num(v) / (d(v) (d(v) - 1)), exactly 0 when d(v) < 2: N(v) is the SET of vertices
//                                 joined to v in either direction, d(v) its size and num(v) the number of stored entries
//                                 (u, w), u != w, with both ends in N(v)
// A: n x n, float or int; its values are never read and its diagonal takes no part.  directed false: A's structure is
// symmetric and only its rows are read (checked when A has columns of its own: GrB_INVALID_VALUE otherwise); true: any
// structure, rows and columns are read.  lcc: a float vector of size n, dense afterwards.  desc may be NULL (no field is
// read).  Returns the Info of the call; the optional last argument receives the library's record (edges, triangles,
// closed = the sum of num, wedges = the sum of d (d - 1), the largest degree, the time of the device work).
#ifndef GRB_HIP_ALGORITHM_LCC_HPP_
#define GRB_HIP_ALGORITHM_LCC_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename a>
inline Info lcc(Vector<float>* lcc, const Matrix<a>* A, bool directed, Descriptor* desc, grb_lcc_result* result = NULL) {
  if (lcc == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_lcc(lcc->handle(), A->handle(), directed ? 1 : 0, desc ? desc->handle() : static_cast<grb_descriptor>(NULL),
                         result));
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_LCC_HPP_
