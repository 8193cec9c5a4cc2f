// graphblas/algorithm/bcc.hpp -- biconnected components, articulation points and bridges through the drop-in frontend.  The
// reference has no such driver (its graphblas/algorithm/ stops at bfs, sssp, pr, cc, tc, ...), so this is no shadow of one of
// its headers: the function goes straight to the library's grb_bcc, whose contract is the comment in grb_hip.h.
//   bcc(C, art, A, mode, desc)   C = A's off-diagonal structure with the block number of every edge (GRB_BCC_BLOCKS), or only
//                                the bridges with the same numbers (GRB_BCC_BRIDGES); the blocks are numbered in ascending
//                                order of their smallest edge key (min(u, v), max(u, v));
//                                art(v) = the number of blocks that contain v: >= 2 exactly at the articulation points
// A: n x n, float or int, symmetric in structure (checked when A has columns of its own: GrB_INVALID_VALUE otherwise); its
// values are never read and its diagonal takes no part.  C: n x n and int whatever A's type, or NULL; C may be A when A is
// int.  art: an int vector of size n, dense afterwards, or NULL.  desc may be NULL (no field is read).  Returns the Info of
// the call; the optional last argument receives the library's record (edges, the largest block, blocks, bridges,
// articulation points, components, isolated vertices, the BFS forest's levels, and what the device ran).
#ifndef GRB_HIP_ALGORITHM_BCC_HPP_
#define GRB_HIP_ALGORITHM_BCC_HPP_

#include "graphblas/graphblas.hpp"

namespace graphblas {
namespace algorithm {

template <typename T>
inline Info bcc(Matrix<int>* C, Vector<int>* art, const Matrix<T>* A, int mode, Descriptor* desc, grb_bcc_result* result = NULL) {
  if (A == NULL) return GrB_UNINITIALIZED_OBJECT;
  return to_info(grb_bcc(C ? C->handle() : static_cast<grb_matrix>(NULL), art ? art->handle() : static_cast<grb_vector>(NULL),
                         A->handle(), mode, desc ? desc->handle() : static_cast<grb_descriptor>(NULL), result));
}

// a non-const A
template <typename T>
inline Info bcc(Matrix<int>* C, Vector<int>* art, Matrix<T>* A, int mode, Descriptor* desc, grb_bcc_result* result = NULL) {
  return bcc<T>(C, art, static_cast<const Matrix<T>*>(A), mode, desc, result);
}

}  // namespace algorithm
}  // namespace graphblas

#endif  // GRB_HIP_ALGORITHM_BCC_HPP_
