// Test driver: the unmasked product through the drop-in frontend (graphblas::mxm with a GrB_NULL mask).
// Reads an .mtx file with readMtx, computes C = A (+.x) A with PlusMultipliesSemiring<float> and prints
// A's and C's CSR, a line each, so tests/test_gpu_spgemm_unmasked.py can compare the product with scipy's A.A.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"

// one line: "csr nrows ncols nvals | row pointers | column indices | values"
static void print_csr(grb_matrix m) {
  grb_index nr = 0, nc = 0, nv = 0;
  const grb_index *ptr, *ind;
  const void* val;
  grb_matrix_nrows(m, &nr);
  grb_matrix_ncols(m, &nc);
  grb_matrix_nvals(m, &nv);
  if (grb_matrix_host_csr(m, &ptr, &ind, &val) != 0) return;
  printf("csr %d %d %d |", nr, nc, nv);
  for (grb_index i = 0; i <= nr; ++i) printf(" %d", ptr[i]);
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
  Matrix<float> a(nr, nc), prod(nr, nc);
  if (a.build(&r, &c, &v, nv, GrB_NULL) != GrB_SUCCESS) return 3;
  Descriptor desc;
  if (mxm<float, float, float, float>(&prod, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<float>(), &a, &a, &desc) != GrB_SUCCESS)
    return 4;
  print_csr(a.handle());
  print_csr(prod.handle());
  return 0;
}
