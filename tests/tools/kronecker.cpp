// Test driver: the kronecker overload through the drop-in frontend, on a 2 x 2 and a 2 x 3 literal.
//   A = [ 1 2 ]      B = [ 1 . 2 ]
//       [ . 3 ]          [ . 3 . ]
// Prints "kron" / "kronT" (the CSR and the CSC of A (x) B under PlusMultiplies: the products) and "minplus" (the CSR under
// MinimumPlus, whose multiply is plus: the sums) as tests/tools/select.cpp prints a side.  tests/test_gpu_kronecker.py
// checks the lines.
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

int main() {
  using namespace graphblas;
  const Index ar[] = {0, 0, 1}, ac[] = {0, 1, 1}, br[] = {0, 0, 1}, bc[] = {0, 2, 1};
  const float av[] = {1, 2, 3}, bv[] = {1, 2, 3};
  std::vector<Index> ra(ar, ar + 3), ca(ac, ac + 3), rb(br, br + 3), cb(bc, bc + 3);
  std::vector<float> va(av, av + 3), vb(bv, bv + 3);
  Matrix<float> a(2, 2), b(2, 3), k(4, 6), s(4, 6);
  if (a.build(&ra, &ca, &va, 3, GrB_NULL) != GrB_SUCCESS) return 3;
  if (b.build(&rb, &cb, &vb, 3, GrB_NULL) != GrB_SUCCESS) return 4;
  Descriptor desc;
  if (kronecker<float, float, float, float>(&k, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<float>(), &a, &b, &desc) != GrB_SUCCESS)
    return 5;
  print_side("kron", k.handle(), false);
  print_side("kronT", k.handle(), true);
  if (kronecker(&s, static_cast<const Matrix<float>*>(NULL), GrB_NULL, MinimumPlusSemiring<float>(), &a, &b, &desc) != GrB_SUCCESS)
    return 6;
  print_side("minplus", s.handle(), false);
  return 0;
}
