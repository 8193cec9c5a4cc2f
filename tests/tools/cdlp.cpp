// Test driver: algorithm::cdlp through the drop-in frontend.
//   "und"   two triangles 0 - 1 - 2 and 3 - 4 - 5 joined by the edge 2 - 3, vertex 6 isolated; a float matrix whose values
//           are zeros and negatives, init NULL, at most 10 iterations: the labels, and "rec" = iterations, changed,
//           evaluated and communities of that call
//   "dir"   the edges 0 -> 1, 0 -> 3, 3 -> 0 on 4 vertices (a const int matrix), directed, one iteration: 3 0 2 0 (vertex 0
//           has 3 twice and 1 once), and "row" = the same matrix undirected, rows only: 1 1 2 0
//   "init"  the first graph again from the labels 6 0 0 3 3 6 1 in place (labels is init), a NULL descriptor
// tests/test_gpu_cdlp.py checks the lines against its reference.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/cdlp.hpp"

static int print_vector(const char* tag, graphblas::Vector<int>* v, int n) {
  std::vector<int> h(n, -1);
  graphblas::Index size = n;
  if (v->extractTuples(&h, &size) != graphblas::GrB_SUCCESS) return 1;
  printf("%s", tag);
  for (int i = 0; i < n; ++i) printf(" %d", h[i]);
  printf("\n");
  return 0;
}

int main() {
  using namespace graphblas;
  const int e[][2] = {{0, 1}, {0, 2}, {1, 2}, {3, 4}, {3, 5}, {4, 5}, {2, 3}};
  std::vector<Index> r, c;
  std::vector<float> vf;
  for (size_t i = 0; i < sizeof(e) / sizeof(e[0]); ++i) {
    r.push_back(e[i][0]); c.push_back(e[i][1]); vf.push_back(0.f);      // stored zeros: edges like any other
    r.push_back(e[i][1]); c.push_back(e[i][0]); vf.push_back(-2.f);
  }
  Matrix<float> a(7, 7);
  if (a.build(&r, &c, &vf, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> labels(7);
  Descriptor desc;
  grb_cdlp_result rec;
  if (algorithm::cdlp(&labels, &a, static_cast<const Vector<int>*>(NULL), false, 10, &desc, &rec) != GrB_SUCCESS) return 4;
  if (print_vector("und", &labels, 7)) return 4;
  printf("rec %d %d %d %d\n", rec.iterations, rec.changed, static_cast<int>(rec.evaluated), rec.communities);

  std::vector<Index> dr, dc;
  std::vector<int> dv;
  const int d[][2] = {{0, 1}, {0, 3}, {3, 0}};
  for (size_t i = 0; i < sizeof(d) / sizeof(d[0]); ++i) { dr.push_back(d[i][0]); dc.push_back(d[i][1]); dv.push_back(static_cast<int>(i) - 1); }
  Matrix<int> b(4, 4);
  if (b.build(&dr, &dc, &dv, static_cast<Index>(dr.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  const Matrix<int>* cb = &b;
  Vector<int> l4(4);
  if (algorithm::cdlp(&l4, cb, static_cast<const Vector<int>*>(NULL), true, 1, &desc) != GrB_SUCCESS) return 5;
  if (print_vector("dir", &l4, 4)) return 5;
  if (algorithm::cdlp(&l4, cb, static_cast<const Vector<int>*>(NULL), false, 1, &desc) != GrB_SUCCESS) return 6;
  if (print_vector("row", &l4, 4)) return 6;

  std::vector<int> start;
  const int s0[] = {6, 0, 0, 3, 3, 6, 1};
  start.assign(s0, s0 + 7);
  Vector<int> io(7);
  if (io.build(&start, 7) != GrB_SUCCESS) return 3;
  if (algorithm::cdlp(&io, &a, &io, false, 10, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 7;
  if (print_vector("init", &io, 7)) return 7;
  return 0;
}
