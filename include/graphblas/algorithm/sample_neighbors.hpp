// graphblas/algorithm/sample_neighbors.hpp -- fan-out-limited neighbour sampling through the drop-in frontend.  The reference
// has no such driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its
// headers: the function goes straight to the library's grb_sample_neighbors, whose contract is the comment in grb_hip.h.
//   sample_neighbors(C, A, seeds, fanout, seed, desc)
//       row k of C = row seeds[k] of A whole when its length d <= fanout, else the fanout entries with the smallest
//       draw(seed, k, p), p the entry's position in the row: uniform without replacement, the same bits on any number of CUs
// A: nrows x ncols, float or int.  seeds: row numbers in any order, duplicates allowed (each is sampled independently); NULL is
// the empty list.  C: ns x ncols of A's type; the kept entries stay in stored order with their value bits; C may be A.  desc
// may be NULL (no field is read).  Returns the Info of the call; the optional last argument receives the library's record
// (rows, entries, full_rows, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_SAMPLE_NEIGHBORS_HPP_
#define GRB_HIP_ALGORITHM_SAMPLE_NEIGHBORS_HPP_

#include <vector>

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info sample_neighbors(Matrix<T>* C, const Matrix<T>* A, const std::vector<Index>* seeds, int fanout, unsigned int seed,
                             Descriptor* desc, grb_sample_result* result = NULL) {
  if (C == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  const bool any = seeds != NULL && !seeds->empty();
  return to_info(grb_sample_neighbors(C->handle(), A->handle(), any ? seeds->data() : static_cast<const grb_index*>(NULL),
                                      any ? static_cast<grb_index>(seeds->size()) : 0, fanout, static_cast<uint32_t>(seed),
                                      desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A
template <typename T>
inline Info sample_neighbors(Matrix<T>* C, Matrix<T>* A, const std::vector<Index>* seeds, int fanout, unsigned int seed,
                             Descriptor* desc, grb_sample_result* result = NULL) {
  return sample_neighbors<T>(C, static_cast<const Matrix<T>*>(A), seeds, fanout, seed, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_SAMPLE_NEIGHBORS_HPP_
