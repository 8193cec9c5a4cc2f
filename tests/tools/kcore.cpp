// Test driver: algorithm::coreness and algorithm::kcore through the drop-in frontend.  It checks its own expected values
// and returns non-zero on a mismatch (the number says which).
//   "bridge"  two triangles 0 - 1 - 2 and 3 - 4 - 5 joined by the edge 2 - 3, vertex 6 pendant on 5, vertex 7 isolated; a
//             float matrix whose values are zeros and negatives.  core = 2 2 2 2 2 2 1 0; the 2-core keeps the six
//             triangle vertices with degrees 2 2 3 3 2 2
//   "k5"      a K5 on 0 .. 4 with the tail 4 - 5 - 6 - 7, a const int matrix with a stored diagonal entry and a NULL
//             descriptor.  core = 4 4 4 4 4 1 1 1; the 3-core is the K5 with degrees 4; the 5-core is empty
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/kcore.hpp"

static bool same(graphblas::Vector<int>* v, const int* want, int n, const char* tag) {
  std::vector<int> h(n, -1);
  graphblas::Index size = n;
  if (v->extractTuples(&h, &size) != graphblas::GrB_SUCCESS || size != n) return false;
  printf("%s", tag);
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    printf(" %d", h[i]);
    ok = ok && h[i] == want[i];
  }
  printf("\n");
  return ok;
}

int main() {
  using namespace graphblas;
  const int e[][2] = {{0, 1}, {0, 2}, {1, 2}, {3, 4}, {3, 5}, {4, 5}, {2, 3}, {5, 6}};
  std::vector<Index> r, c;
  std::vector<float> vf;
  for (size_t i = 0; i < sizeof(e) / sizeof(e[0]); ++i) {
    r.push_back(e[i][0]); c.push_back(e[i][1]); vf.push_back(0.f);      // stored zeros: edges like any other
    r.push_back(e[i][1]); c.push_back(e[i][0]); vf.push_back(-2.f);
  }
  Matrix<float> a(8, 8);
  if (a.build(&r, &c, &vf, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> core(8);
  Descriptor desc;
  grb_kcore_result rec;
  if (algorithm::coreness(&core, &a, &desc, &rec) != GrB_SUCCESS) return 4;
  const int want_core[8] = {2, 2, 2, 2, 2, 2, 1, 0};
  if (!same(&core, want_core, 8, "bridge core")) return 5;
  if (rec.edges != 8 || rec.kmax != 2 || rec.levels != 3 || rec.result_vertices != 6 || rec.result_edges != 7 || rec.launches < 1) return 6;
  Vector<int> in2(8);
  if (algorithm::kcore(&in2, &a, 2, &desc, &rec) != GrB_SUCCESS) return 7;
  const int want_in2[8] = {2, 2, 3, 3, 2, 2, 0, 0};
  if (!same(&in2, want_in2, 8, "bridge 2-core")) return 8;
  if (rec.edges != 8 || rec.kmax != 2 || rec.levels != 1 || rec.result_vertices != 6 || rec.result_edges != 7) return 9;
  if (algorithm::kcore(&in2, &a, -1, &desc) != GrB_INVALID_VALUE) return 10;
  if (!same(&in2, want_in2, 8, "bridge unchanged")) return 11;

  std::vector<Index> kr, kc;
  std::vector<int> kv;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j)
      if (i != j) { kr.push_back(i); kc.push_back(j); kv.push_back(i - j); }
  const int tail[][2] = {{4, 5}, {5, 6}, {6, 7}};
  for (size_t i = 0; i < 3; ++i) {
    kr.push_back(tail[i][0]); kc.push_back(tail[i][1]); kv.push_back(0);
    kr.push_back(tail[i][1]); kc.push_back(tail[i][0]); kv.push_back(0);
  }
  kr.push_back(5); kc.push_back(5); kv.push_back(9);                     // a diagonal entry: no part
  Matrix<int> b(8, 8);
  if (b.build(&kr, &kc, &kv, static_cast<Index>(kr.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  const Matrix<int>* cb = &b;
  Vector<int> c5(8);
  grb_kcore_result krec;
  if (algorithm::coreness(&c5, cb, static_cast<Descriptor*>(NULL), &krec) != GrB_SUCCESS) return 12;
  const int want_c5[8] = {4, 4, 4, 4, 4, 1, 1, 1};
  if (!same(&c5, want_c5, 8, "k5 core")) return 13;
  if (krec.edges != 13 || krec.kmax != 4 || krec.levels != 2 || krec.result_vertices != 5 || krec.result_edges != 10) return 14;
  Vector<int> in3(8);
  if (algorithm::kcore(&in3, cb, 3, static_cast<Descriptor*>(NULL), &krec) != GrB_SUCCESS) return 15;
  const int want_in3[8] = {4, 4, 4, 4, 4, 0, 0, 0};
  if (!same(&in3, want_in3, 8, "k5 3-core")) return 16;
  if (krec.result_vertices != 5 || krec.result_edges != 10 || krec.kmax != 3) return 17;
  if (algorithm::kcore(&in3, cb, 5, static_cast<Descriptor*>(NULL), &krec) != GrB_SUCCESS) return 18;
  const int zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!same(&in3, zeros, 8, "k5 5-core")) return 19;
  if (krec.result_vertices != 0 || krec.result_edges != 0 || krec.kmax != 5) return 20;
  if (algorithm::kcore(&in3, cb, 0, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 21;
  const int degs[8] = {4, 4, 4, 4, 5, 2, 2, 1};
  if (!same(&in3, degs, 8, "k5 degrees")) return 22;
  printf("ok\n");
  return 0;
}
