// Test driver: algorithm::ktruss and algorithm::trussness through the drop-in frontend, on K4 with a pendant triangle and
// a pendant edge (7 vertices):
//   0 - 1 - 2 - 3 all joined (K4); 3 - 4, 3 - 5, 4 - 5 (a triangle hanging on 3); 5 - 6 (an edge in no triangle)
// Prints "k4" (the CSR of the 4-truss, int supports: K4 with 2 everywhere), "k3T" (the CSC of the 3-truss into a float
// matrix), "truss" (the trussness of every edge) and "rec" (rounds > 0, edges, result edges and kmax of the trussness call)
// as tests/tools/kronecker.cpp prints a side.  tests/test_gpu_ktruss.py checks the lines.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/ktruss.hpp"

template <typename T>
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
  for (grb_index i = 0; i < nv; ++i) printf(" %.9g", static_cast<double>(static_cast<const T*>(val)[i]));
  printf("\n");
}

int main() {
  using namespace graphblas;
  const int e[][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}, {3, 4}, {3, 5}, {4, 5}, {5, 6}};
  std::vector<Index> r, c;
  std::vector<float> v;
  for (size_t i = 0; i < sizeof(e) / sizeof(e[0]); ++i) {
    r.push_back(e[i][0]); c.push_back(e[i][1]); v.push_back(0.f);       // stored zeros: edges like any other
    r.push_back(e[i][1]); c.push_back(e[i][0]); v.push_back(-1.f);
  }
  Matrix<float> a(7, 7), k3(7, 7);
  Matrix<int> k4(7, 7), t(7, 7);
  if (a.build(&r, &c, &v, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Descriptor desc;
  if (algorithm::ktruss(&k4, &a, 4, &desc) != GrB_SUCCESS) return 4;
  print_side<int>("k4", k4.handle(), false);
  const Matrix<float>* ca = &a;
  if (algorithm::ktruss(&k3, ca, 3, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 5;
  print_side<float>("k3T", k3.handle(), true);
  grb_truss_result rec;
  if (algorithm::trussness(&t, ca, &desc, &rec) != GrB_SUCCESS) return 6;
  print_side<int>("truss", t.handle(), false);
  printf("rec %d %d %d %d\n", rec.rounds > 0 ? 1 : 0, static_cast<int>(rec.edges), static_cast<int>(rec.result_edges), rec.kmax);
  return 0;
}
