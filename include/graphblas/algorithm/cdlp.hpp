// graphblas/algorithm/cdlp.hpp -- community detection by label propagation through the drop-in frontend.  The reference
// has no such driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its
// headers: the function goes straight to the library's grb_cdlp, whose contract is the comment in grb_hip.h.
//   cdlp(labels, A, init, directed, max_iter, desc)   synchronous CDLP: every vertex takes the most frequent label among
//                                                     its neighbours, the smallest one on a tie, until nothing changes
//                                                     or max_iter iterations have run
// A: n x n, float or int; its values are never read and its diagonal takes no part.  directed false: a vertex's
// neighbours are the columns stored in its row; true: those plus the rows stored in its column (a vertex joined both ways
// counts twice).  init: the starting labels, an int vector of size n with all n values stored, each in 0 .. n - 1, or NULL
// for L(v) = v.  labels: an int vector of size n, dense afterwards; it may be init.  desc may be NULL (no field is read).
// Returns the Info of the call; the optional last argument receives the library's record (iterations, labels the last
// iteration changed, modes computed, distinct labels, the time of the loop).
#ifndef GRB_HIP_ALGORITHM_CDLP_HPP_
#define GRB_HIP_ALGORITHM_CDLP_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename a>
inline Info cdlp(Vector<int>* labels, const Matrix<a>* A, const Vector<int>* init, bool directed, int max_iter, Descriptor* desc,
                 grb_cdlp_result* result = NULL) {
  if (labels == NULL || A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_cdlp(labels->handle(), A->handle(), init ? init->handle() : static_cast<grb_vector>(NULL), directed ? 1 : 0,
                          max_iter, desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_CDLP_HPP_
