// Test driver: the three extract forms through the drop-in frontend, on a 4 x 4 literal.
//       0 1 2 3
//   0 [ 1 . 2 . ]
//   1 [ . 3 . . ]      (the value 0 at (3, 1) is a stored zero)
//   2 [ 4 . 5 6 ]
//   3 [ . 0 . 7 ]
// Prints "csr"/"csc" lines of C = A({2, 0, 2}, {3, 0}) as tests/tools/ewise_matrix.cpp prints them, then "col" (column 0
// of A at rows {2, 1, 0, 0}), "row" (row 2 of A under GrB_INP0 = GrB_TRAN, every column) and "sub" (u({3, 3, 0}) of a
// dense u): "<tag> n | indices | values".  tests/test_gpu_extract.py checks the lines.
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
  Matrix<float> a(4, 4), sub(3, 2);
  if (a.build(&r, &c, &v, 8, GrB_NULL) != GrB_SUCCESS) return 3;
  Descriptor desc;
  const Index ii[] = {2, 0, 2}, jj[] = {3, 0};
  std::vector<Index> I(ii, ii + 3), J(jj, jj + 2);
  if (extract<float, float, float>(&sub, GrB_NULL, GrB_NULL, &a, &I, 3, &J, 2, &desc) != GrB_SUCCESS) return 4;
  print_side("csr", sub.handle(), false);
  print_side("csc", sub.handle(), true);
  const Index kk[] = {2, 1, 0, 0};
  std::vector<Index> K(kk, kk + 4);
  Vector<float> col(4), row(4), u(4), w(3);
  if (extract<float, float, float>(&col, GrB_NULL, GrB_NULL, &a, &K, 4, 0, &desc) != GrB_SUCCESS) return 5;
  if (print_sparse("col", &col)) return 6;
  if (desc.toggle(GrB_INP0) != GrB_SUCCESS) return 7;
  if (extract<float, float, float>(&row, GrB_NULL, GrB_NULL, &a, GrB_ALL, 4, 2, &desc) != GrB_SUCCESS) return 8;
  if (desc.toggle(GrB_INP0) != GrB_SUCCESS) return 7;
  if (print_sparse("row", &row)) return 9;
  std::vector<float> uv(4);
  for (int i = 0; i < 4; ++i) uv[i] = 10.f + i;
  if (u.build(&uv, 4) != GrB_SUCCESS) return 10;
  const Index ss[] = {3, 3, 0};
  std::vector<Index> S(ss, ss + 3);
  if (extract<float, float, float>(&w, GrB_NULL, GrB_NULL, &u, &S, 3, &desc) != GrB_SUCCESS) return 11;
  std::vector<float> wv;
  Index n = 3;
  if (w.extractTuples(&wv, &n) != GrB_SUCCESS) return 12;
  printf("sub %d | | %.9g %.9g %.9g\n", n, wv[0], wv[1], wv[2]);
  return 0;
}
