// Test driver: algorithm::scc through the drop-in frontend.  It checks its own expected values and returns non-zero on a
// mismatch (the number says which).
//   "bowtie"  the cycles 1 -> 2 -> 3 -> 1 and 4 -> 5 -> 6 -> 4 joined by the one-way edge 3 -> 4, vertex 0 with the edge
//             0 -> 1 only, vertex 7 isolated; a float matrix whose values are zeros and negatives.
//             scc = 0 1 1 1 4 4 4 7; 4 components, the largest 3, 2 of one vertex
//   "ring"    the cycle 7 -> 6 -> ... -> 0 -> 7 with a chord 2 -> 5, a const int matrix with a stored diagonal entry and a
//             NULL descriptor.  scc = 0 everywhere; 1 component
//   "dag"     the edges i -> j for every i < j of 6 vertices: trimming alone, rounds = 0
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/scc.hpp"

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
  const int e[][2] = {{1, 2}, {2, 3}, {3, 1}, {4, 5}, {5, 6}, {6, 4}, {3, 4}, {0, 1}};
  std::vector<Index> r, c;
  std::vector<float> vf;
  for (size_t i = 0; i < sizeof(e) / sizeof(e[0]); ++i) {
    r.push_back(e[i][0]); c.push_back(e[i][1]); vf.push_back(i & 1 ? 0.f : -2.f);   // stored zeros: edges like any other
  }
  Matrix<float> a(8, 8);
  if (a.build(&r, &c, &vf, static_cast<Index>(r.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> comp(8);
  Descriptor desc;
  grb_scc_result rec;
  if (algorithm::scc(&comp, &a, &desc, &rec) != GrB_SUCCESS) return 4;
  const int want_bowtie[8] = {0, 1, 1, 1, 4, 4, 4, 7};
  if (!same(&comp, want_bowtie, 8, "bowtie scc")) return 5;
  if (rec.edges != 8 || rec.components != 4 || rec.largest != 3 || rec.trivial != 2 || rec.launches != 1) return 6;
  Vector<int> wrong(7);
  if (algorithm::scc(&wrong, &a, &desc) != GrB_DIMENSION_MISMATCH) return 7;
  if (!same(&comp, want_bowtie, 8, "bowtie unchanged")) return 8;

  std::vector<Index> kr, kc;
  std::vector<int> kv;
  for (int i = 0; i < 8; ++i) { kr.push_back(i); kc.push_back((i + 7) % 8); kv.push_back(i - 3); }
  kr.push_back(2); kc.push_back(5); kv.push_back(0);
  kr.push_back(5); kc.push_back(5); kv.push_back(9);                     // a diagonal entry: no part
  Matrix<int> b(8, 8);
  if (b.build(&kr, &kc, &kv, static_cast<Index>(kr.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  const Matrix<int>* cb = &b;
  Vector<int> ring(8);
  grb_scc_result rrec;
  if (algorithm::scc(&ring, cb, static_cast<Descriptor*>(NULL), &rrec) != GrB_SUCCESS) return 9;
  const int zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!same(&ring, zeros, 8, "ring scc")) return 10;
  if (rrec.edges != 9 || rrec.components != 1 || rrec.largest != 8 || rrec.trivial != 0 || rrec.launches != 1) return 11;

  std::vector<Index> dr, dc;
  std::vector<float> dv;
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j) { dr.push_back(i); dc.push_back(j); dv.push_back(1.f); }
  Matrix<float> d(6, 6);
  if (d.build(&dr, &dc, &dv, static_cast<Index>(dr.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> dag(6);
  grb_scc_result drec;
  if (algorithm::scc(&dag, &d, &desc, &drec) != GrB_SUCCESS) return 12;
  const int ident[6] = {0, 1, 2, 3, 4, 5};
  if (!same(&dag, ident, 6, "dag scc")) return 13;
  if (drec.edges != 15 || drec.components != 6 || drec.largest != 1 || drec.trivial != 6 || drec.rounds != 0 || drec.trimmed != 6) return 14;
  printf("ok\n");
  return 0;
}
