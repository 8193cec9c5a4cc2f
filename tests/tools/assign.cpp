// Test driver: the four matrix assign forms through the drop-in frontend, on the 4 x 4 literal of tests/tools/extract.cpp.
//       0 1 2 3
//   0 [ 1 . 2 . ]
//   1 [ . 3 . . ]      (the value 0 at (3, 1) is a stored zero)
//   2 [ 4 . 5 6 ]
//   3 [ . 0 . 7 ]
// One call of each form on a fresh copy of it, "csr" / "csc" lines after each as tests/tools/extract.cpp prints them:
//   mat  C({2, 0}, {3, 0}) = B, B = [[10 .] [. 20]], no accum       const  C({1, 3}, ALL) = 9 with plus as the accum
//   col  C({3, 1}, 2) = u, u = {30, 40} dense, no accum             row    C(2, {0, 1}) = s, s = {1: 50} sparse, no accum
// tests/test_gpu_assign.py checks the lines.
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

static int fresh(graphblas::Matrix<float>* a) {
  using namespace graphblas;
  const Index rr[] = {0, 0, 1, 2, 2, 2, 3, 3}, cc[] = {0, 2, 1, 0, 2, 3, 1, 3};
  const float vv[] = {1, 2, 3, 4, 5, 6, 0, 7};
  std::vector<Index> r(rr, rr + 8), c(cc, cc + 8);
  std::vector<float> v(vv, vv + 8);
  return a->build(&r, &c, &v, 8, GrB_NULL) == GrB_SUCCESS ? 0 : 1;
}

int main() {
  using namespace graphblas;
  Descriptor desc;
  const std::vector<Index>* all = NULL;
  {
    Matrix<float> c(4, 4), b(2, 2);
    if (fresh(&c)) return 3;
    std::vector<Index> br(2), bc(2);
    std::vector<float> bv(2);
    br[0] = 0; bc[0] = 0; bv[0] = 10.f;
    br[1] = 1; bc[1] = 1; bv[1] = 20.f;
    if (b.build(&br, &bc, &bv, 2, GrB_NULL) != GrB_SUCCESS) return 3;
    const Index ii[] = {2, 0}, jj[] = {3, 0};
    std::vector<Index> I(ii, ii + 2), J(jj, jj + 2);
    if (assign<float, float, float>(&c, GrB_NULL, GrB_NULL, &b, &I, 2, &J, 2, &desc) != GrB_SUCCESS) return 4;
    print_side("csr mat", c.handle(), false);
    print_side("csc mat", c.handle(), true);
  }
  {
    Matrix<float> c(4, 4);
    if (fresh(&c)) return 3;
    const Index ii[] = {1, 3};
    std::vector<Index> I(ii, ii + 2);
    if (assign<float, float, float>(&c, GrB_NULL, graphblas::plus<float>(), 9.f, &I, 2, all, 4, &desc) != GrB_SUCCESS) return 5;
    print_side("csr const", c.handle(), false);
    print_side("csc const", c.handle(), true);
  }
  {
    Matrix<float> c(4, 4);
    if (fresh(&c)) return 3;
    Vector<float> u(2);
    std::vector<float> uv(2);
    uv[0] = 30.f; uv[1] = 40.f;
    if (u.build(&uv, 2) != GrB_SUCCESS) return 6;
    const Index ii[] = {3, 1};
    const std::vector<Index> I(ii, ii + 2);
    const Index col = 2;
    if (assign<float, float, float>(&c, GrB_NULL, GrB_NULL, &u, &I, 2, col, &desc) != GrB_SUCCESS) return 7;
    print_side("csr col", c.handle(), false);
    print_side("csc col", c.handle(), true);
  }
  {
    Matrix<float> c(4, 4);
    if (fresh(&c)) return 3;
    Vector<float> s(2);
    std::vector<Index> si(1, 1);
    std::vector<float> sv(1, 50.f);
    if (s.build(&si, &sv, 1, GrB_NULL) != GrB_SUCCESS) return 8;
    const Index jj[] = {0, 1};
    const std::vector<Index> J(jj, jj + 2);
    const Index row = 2;
    if (assign<float, float, float>(&c, GrB_NULL, GrB_NULL, &s, row, &J, 2, &desc) != GrB_SUCCESS) return 9;
    print_side("csr row", c.handle(), false);
    print_side("csc row", c.handle(), true);
  }
  return 0;
}
