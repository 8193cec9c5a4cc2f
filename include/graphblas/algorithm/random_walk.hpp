// graphblas/algorithm/random_walk.hpp -- random walks through the drop-in frontend.  The reference has no such driver (its
// graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the function goes
// straight to the library's grb_random_walk, whose contract is the comment in grb_hip.h.
//   random_walk(walks, A, starts, length, mode, seed, desc)
//       walks[w * (length + 1) + t] = walker w's vertex after t steps, -1 behind a dead end; step t of walker w draws
//       draw(seed, w, t), a pure function: the same bits on any number of CUs
// A: n x n, float or int, directed or not; a stored A(i, j) is the step i -> j.  starts: vertex ids (duplicates are
// different walkers), or NULL for every vertex in order.  mode = GRB_WALK_UNIFORM never reads the values; mode =
// GRB_WALK_WEIGHTED reads them as weights (int >= 0; float a non-negative integer value <= 2^24; every row sum <= 2^31 - 1).
// walks: an int vector of size ns * (length + 1), dense afterwards.  desc may be NULL (no field is read).  Returns the Info of
// the call; the optional last argument receives the library's record (walkers, steps, dead_ends, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_RANDOM_WALK_HPP_
#define GRB_HIP_ALGORITHM_RANDOM_WALK_HPP_

#include <vector>

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info random_walk(Vector<int>* walks, const Matrix<T>* A, const std::vector<Index>* starts, int length, int mode,
                        unsigned int seed, Descriptor* desc, grb_walk_result* result = NULL) {
  if (walks == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  static const grb_index none = 0;                       // an empty list is no walkers, not "every vertex"
  const grb_index* list = !starts ? static_cast<const grb_index*>(NULL) : starts->empty() ? &none : starts->data();
  const int64_t ns = starts ? static_cast<int64_t>(starts->size()) : 0;
  return to_info(grb_random_walk(walks->handle(), A->handle(), list, ns, length, mode, static_cast<uint32_t>(seed),
                                 desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A
template <typename T>
inline Info random_walk(Vector<int>* walks, Matrix<T>* A, const std::vector<Index>* starts, int length, int mode,
                        unsigned int seed, Descriptor* desc, grb_walk_result* result = NULL) {
  return random_walk<T>(walks, static_cast<const Matrix<T>*>(A), starts, length, mode, seed, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_RANDOM_WALK_HPP_
