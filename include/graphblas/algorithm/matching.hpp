// graphblas/algorithm/matching.hpp -- greedy weighted and maximal matching through the drop-in frontend.  The reference has
// no such driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers:
// the function goes straight to the library's grb_matching, whose contract is the comment in grb_hip.h.
//   matching(mate, C, A, mode, seed, desc)   mate(v) = v's partner, or -1, in the matching the greedy scan builds when it takes
//                                            the edges in the order of the key (p, min(u, v), max(u, v)) and keeps an edge
//                                            when both ends are still free; C = both directions of every matched edge with
//                                            A's bits from the row of min(u, v)
// mode: GRB_MATCH_HEAVIEST (0, p = the weight descending), GRB_MATCH_LIGHTEST (1, ascending) or GRB_MATCH_HASHED (2, a hash of
// the two ends and seed; the values are not read).  A: n x n, float or int, symmetric (checked when A has columns of its own:
// GrB_INVALID_VALUE otherwise, as is a NaN off the diagonal in modes 0 and 1); its diagonal takes no part.  mate: an int
// vector of size n, dense afterwards.  C: NULL, or n x n of A's type; C may be A.  desc may be NULL (no field is read).
// Returns the Info of the call; the optional last argument receives the library's record (edges, the matching's edges and
// weight, the exposed and the isolated vertices, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_MATCHING_HPP_
#define GRB_HIP_ALGORITHM_MATCHING_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info matching(Vector<int>* mate, Matrix<T>* C, const Matrix<T>* A, int mode, unsigned int seed, Descriptor* desc,
                     grb_matching_result* result = NULL) {
  if (mate == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_matching(mate->handle(), C ? C->handle() : static_cast<grb_matrix>(NULL), A->handle(), mode, seed,
                              desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A (the template argument is deduced from C and A alike)
template <typename T>
inline Info matching(Vector<int>* mate, Matrix<T>* C, Matrix<T>* A, int mode, unsigned int seed, Descriptor* desc,
                     grb_matching_result* result = NULL) {
  return matching<T>(mate, C, static_cast<const Matrix<T>*>(A), mode, seed, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_MATCHING_HPP_
