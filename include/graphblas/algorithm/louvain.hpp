// graphblas/algorithm/louvain.hpp -- Louvain community detection through the drop-in frontend.  The reference has no such
// driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the
// function goes straight to the library's grb_louvain, whose contract is the comment in grb_hip.h.
//   louvain(labels, A, weighted, max_levels, max_rounds, desc)
//       labels(v) = the smallest original vertex number in v's community after deterministic Louvain modularity optimisation
//       in exact integers: propose / claim / accept rounds, then grb_relabel and grb_contract between the levels
// A: n x n, float or int, symmetric in structure and values (checked when A has columns of its own: GrB_INVALID_VALUE
// otherwise).  weighted = 1 reads the values (int >= 0; float a non-negative integer value <= 2^24), weighted = 0 gives every
// stored entry weight 1; the sum of all stored weights must be <= 2^31 - 1.  labels: an int vector of size n, dense
// afterwards.  desc may be NULL (no field is read).  Returns the Info of the call; the optional last argument receives the
// library's record (levels, rounds, moves, proposals, communities, qn, w, modularity, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_LOUVAIN_HPP_
#define GRB_HIP_ALGORITHM_LOUVAIN_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info louvain(Vector<int>* labels, const Matrix<T>* A, int weighted, int max_levels, int max_rounds, Descriptor* desc,
                    grb_louvain_result* result = NULL) {
  if (labels == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_louvain(labels->handle(), A->handle(), weighted, max_levels, max_rounds,
                             desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A
template <typename T>
inline Info louvain(Vector<int>* labels, Matrix<T>* A, int weighted, int max_levels, int max_rounds, Descriptor* desc,
                    grb_louvain_result* result = NULL) {
  return louvain<T>(labels, static_cast<const Matrix<T>*>(A), weighted, max_levels, max_rounds, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_LOUVAIN_HPP_
