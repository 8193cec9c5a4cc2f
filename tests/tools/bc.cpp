// Test driver: algorithm::bc through the drop-in frontend, on the graph of tests/golden/data/test_bc.mtx (7 vertices, 15
// directed edges; the entry "r c" of the file is the edge r - 1 -> c - 1).  Prints "all" (every vertex a source: a NULL
// list, a NULL descriptor, a float matrix), "list" (the explicit list 0 .. 6 on a const int matrix whose values are zeros
// and negatives), "two" (the sources 2 and 2: a source listed twice counts twice) -- seven values each -- and "rec"
// (sources, batches, levels and vertices reached of the first call).  tests/test_gpu_bc.py checks the lines.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/bc.hpp"

static int print_vector(const char* tag, graphblas::Vector<float>* v) {
  std::vector<float> h(7, -1.f);
  graphblas::Index n = 7;
  if (v->extractTuples(&h, &n) != graphblas::GrB_SUCCESS) return 1;
  printf("%s", tag);
  for (int i = 0; i < 7; ++i) printf(" %.9g", static_cast<double>(h[i]));
  printf("\n");
  return 0;
}

int main() {
  using namespace graphblas;
  const int e[][2] = {{2, 1}, {3, 1}, {4, 1}, {1, 2}, {5, 2}, {3, 2}, {4, 3}, {5, 3}, {6, 3}, {6, 4}, {7, 4}, {3, 5}, {6, 5},
                      {7, 5}, {7, 6}};
  std::vector<Index> r, c;
  std::vector<float> vf;
  std::vector<int> vi;
  for (size_t i = 0; i < sizeof(e) / sizeof(e[0]); ++i) {
    r.push_back(e[i][0] - 1); c.push_back(e[i][1] - 1);
    vf.push_back(1.f);
    vi.push_back(i % 2 ? 0 : -3);                         // stored zeros: edges like any other
  }
  Matrix<float> a(7, 7);
  Matrix<int> b(7, 7);
  if (a.build(&r, &c, &vf, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  if (b.build(&r, &c, &vi, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<float> v(7);
  grb_bc_result rec;
  if (algorithm::bc(&v, &a, static_cast<const std::vector<Index>*>(NULL), static_cast<Descriptor*>(NULL), &rec) != GrB_SUCCESS) return 4;
  if (print_vector("all", &v)) return 4;
  Descriptor desc;
  std::vector<Index> src;
  for (Index i = 0; i < 7; ++i) src.push_back(i);
  const Matrix<int>* cb = &b;
  if (algorithm::bc(&v, cb, &src, &desc) != GrB_SUCCESS) return 5;
  if (print_vector("list", &v)) return 5;
  std::vector<Index> two(2, 2);
  if (algorithm::bc(&v, cb, &two, &desc) != GrB_SUCCESS) return 6;
  if (print_vector("two", &v)) return 6;
  printf("rec %d %d %d %d\n", rec.sources, rec.batches, rec.levels, static_cast<int>(rec.reached));
  return 0;
}
