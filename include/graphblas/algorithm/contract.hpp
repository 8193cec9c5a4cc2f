// graphblas/algorithm/contract.hpp -- graph contraction through the drop-in frontend.  The reference has no such driver (its
// graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of its headers: the functions go
// straight to the library's grb_relabel and grb_contract, whose contracts are the comment in grb_hip.h.
//   relabel(map, labels, kind, count)              map(v) = the number of distinct labels smaller than L(v); *count (nullable)
//                                                  = the distinct labels.  kind: GRB_RELABEL_LABELS (0, L = labels, each in
//                                                  0 .. n - 1) or GRB_RELABEL_MATE (1, L(v) = v when labels(v) < 0, otherwise
//                                                  min(v, labels(v)): what matching() writes).  map may be labels.
//   contract(C, sizes, A, map, op, loops, desc)    C = S^T A S with S(v, map(v)) = 1.  A: n x n, float or int, any structure.
//                                                  map: an int vector of size n, every value stored, each in -1 .. nc - 1 for
//                                                  the nc x nc C; -1 drops the vertex.  loops = 0 drops the entries with
//                                                  map(i) = map(j), 1 keeps them.  op: GRB_OP_PLUS (int wraps; float adds in
//                                                  double in a fixed order and rounds once), GRB_OP_MINIMUM, GRB_OP_MAXIMUM
//                                                  (the winner's bits) or GRB_OP_FIRST (the entry with the smallest (i, j)).
//                                                  sizes: NULL, or an int vector of size nc: the vertices mapped to each id.
//                                                  C is of A's type; C may be A when nc = n.  desc may be NULL.
// Both return the Info of the call; contract's optional last argument receives the library's record (kept, loops, entries,
// clusters, dropped, largest, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_CONTRACT_HPP_
#define GRB_HIP_ALGORITHM_CONTRACT_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

inline Info relabel(Vector<int>* map, const Vector<int>* labels, int kind, int* count = NULL) {
  if (map == NULL || labels == NULL) return GrB_UNINITIALIZED_OBJECT;
  int32_t nc = 0;
  const Info info = to_info(grb_relabel(map->handle(), labels->handle(), kind, &nc, static_cast<grb_descriptor>(NULL)));
  if (count != NULL && info == GrB_SUCCESS) *count = static_cast<int>(nc);
  return info;
}

template <typename T>
inline Info contract(Matrix<T>* C, Vector<int>* sizes, const Matrix<T>* A, const Vector<int>* map, grb_binary_op op, int loops,
                     Descriptor* desc, grb_contract_result* result = NULL) {
  if (C == NULL || A == NULL || map == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_contract(C->handle(), sizes ? sizes->handle() : static_cast<grb_vector>(NULL), A->handle(), map->handle(), op, loops,
                              desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A (the template argument is deduced from C and A alike)
template <typename T>
inline Info contract(Matrix<T>* C, Vector<int>* sizes, Matrix<T>* A, const Vector<int>* map, grb_binary_op op, int loops,
                     Descriptor* desc, grb_contract_result* result = NULL) {
  return contract<T>(C, sizes, static_cast<const Matrix<T>*>(A), map, op, loops, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_CONTRACT_HPP_
