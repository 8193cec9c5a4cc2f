// Test driver: the matrix eWiseAdd / eWiseMult and transpose through the drop-in frontend.  Reads an .mtx file with
// readMtx, forms the product P = A (+.x) A (CSR only), then E = P + A, M = P .* A and T = P^T, and prints the CSR of A,
// E, M and T and the CSC of T, a line each, so tests/test_gpu_ewise_matrix.py can compare them with scipy.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"

// one line: "<tag> nrows ncols nvals | pointers | indices | values"
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using namespace graphblas;
  std::vector<Index> r, c;
  std::vector<float> v;
  Index nr, nc, nv;
  readMtx(argv[1], &r, &c, &v, &nr, &nc, &nv, 1, false, NULL);
  Matrix<float> a(nr, nc), prod(nr, nc), sum(nr, nc), both(nr, nc), tr(nc, nr);
  if (a.build(&r, &c, &v, nv, GrB_NULL) != GrB_SUCCESS) return 3;
  Descriptor desc;
  if (mxm<float, float, float, float>(&prod, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<float>(), &a, &a, &desc) != GrB_SUCCESS)
    return 4;
  if (eWiseAdd<float, float, float, float>(&sum, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<float>(), &prod, &a, &desc) != GrB_SUCCESS)
    return 5;
  if (eWiseMult<float, float, float, float>(&both, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<float>(), &prod, &a, &desc) !=
      GrB_SUCCESS)
    return 6;
  if (transpose<float, float, float>(&tr, GrB_NULL, GrB_NULL, &prod, &desc) != GrB_SUCCESS) return 7;
  print_side("csr", a.handle(), false);
  print_side("csr", sum.handle(), false);
  print_side("csr", both.handle(), false);
  print_side("csr", tr.handle(), false);
  print_side("csc", tr.handle(), true);
  return 0;
}
