// Test driver: the two select overloads through the drop-in frontend, on a 4 x 4 literal.
//       0 1 2 3
//   0 [ 1 . 2 . ]
//   1 [ . 3 . . ]      (the value 0 at (3, 1) is a stored zero)
//   2 [ 4 . 5 6 ]
//   3 [ . 0 . 7 ]
// Prints "tril" / "trilT" (the CSR and the CSC of the strictly lower triangle, GrB_SEL_TRIL with thunk -1), "nz" (the CSR
// of A without its stored zero, GrB_SEL_VALUENE 0, in place) as tests/tools/extract.cpp prints a side, then "vgt" (the
// entries > 11 of a dense u = {10, 11, 12, 13}) and "vrow" (the entries of that result at indices <= 2):
// "<tag> n | indices | values".  tests/test_gpu_select.py checks the lines.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"

static void print_side(const char* tag, grb_matrix m, bool csc) {
  grb_index nr = 0, nc = 0, nv = 0;
  const grb_index *ptr, *ind;
  const void* val;
  grb_matrix_nrows(m, &nr);
  grb_matrix_ncols(m, &nc);
  grb_matrix_nvals(m, &nv);
  if ((csc ? grb_matrix_host_csc(m, &ptr, &ind, &val) : grb_matrix_host_csr(m, &ptr, &ind, &val)) != 0) return;
  printf("%s %d %d %d |", tag, nr, nc, nv);
  for (grb_index i = 0; i <= (csc ? nc : nr); ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %.9g", static_cast<const float*>(val)[i]);
  printf("\n");
}

static int print_sparse(const char* tag, graphblas::Vector<float>* w) {
  using namespace graphblas;
  Index n = 0;
  if (w->nvals(&n) != GrB_SUCCESS) return 1;
  std::vector<Index> ind;
  std::vector<float> val;
  if (w->extractTuples(&ind, &val, &n) != GrB_SUCCESS) return 1;
  printf("%s %d |", tag, n);
  for (Index i = 0; i < n; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (Index i = 0; i < n; ++i) printf(" %.9g", val[i]);
  printf("\n");
  return 0;
}

int main() {
  using namespace graphblas;
  const Index rr[] = {0, 0, 1, 2, 2, 2, 3, 3}, cc[] = {0, 2, 1, 0, 2, 3, 1, 3};
  const float vv[] = {1, 2, 3, 4, 5, 6, 0, 7};
  std::vector<Index> r(rr, rr + 8), c(cc, cc + 8);
  std::vector<float> v(vv, vv + 8);
  Matrix<float> a(4, 4), low(4, 4);
  if (a.build(&r, &c, &v, 8, GrB_NULL) != GrB_SUCCESS) return 3;
  Descriptor desc;
  if (select<float, float, float>(&low, GrB_NULL, GrB_NULL, GrB_SEL_TRIL, &a, -1, &desc) != GrB_SUCCESS) return 4;
  print_side("tril", low.handle(), false);
  print_side("trilT", low.handle(), true);
  if (select(&a, static_cast<const Matrix<float>*>(NULL), GrB_NULL, GrB_SEL_VALUENE, &a, 0, &desc) != GrB_SUCCESS) return 5;
  print_side("nz", a.handle(), false);
  Vector<float> u(4), w(4);
  std::vector<float> uv(4);
  for (int i = 0; i < 4; ++i) uv[i] = 10.f + i;
  if (u.build(&uv, 4) != GrB_SUCCESS) return 6;
  if (select<float, float, float>(&w, GrB_NULL, GrB_NULL, GrB_SEL_VALUEGT, &u, 11, &desc) != GrB_SUCCESS) return 7;
  if (print_sparse("vgt", &w)) return 8;
  if (select(&w, static_cast<const Vector<float>*>(NULL), GrB_NULL, GrB_SEL_ROWLE, &w, 2, &desc) != GrB_SUCCESS) return 9;
  if (print_sparse("vrow", &w)) return 10;
  return 0;
}
