// Test driver: algorithm::lcc through the drop-in frontend.
//   "und"   two triangles 0 - 1 - 2 and 3 - 4 - 5 joined by the edge 2 - 3, vertex 6 isolated; a float matrix whose values
//           are zeros and negatives: the values as the hexadecimal bits of their floats, and "rec" = edges, triangles,
//           closed, wedges and max_degree of that call
//   "dir"   the entries 0 -> 1, 1 -> 0, 1 -> 2, 2 -> 0, 0 -> 3, 3 -> 1 and the diagonal entry 3 -> 3 on 5 vertices (a const
//           int matrix), directed, a NULL descriptor: the values, and "drec" = the record
//   "asym"  the same matrix undirected: 1 when the call says GrB_INVALID_VALUE (its structure is not symmetric)
// tests/test_gpu_lcc.py checks the lines against its reference.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/lcc.hpp"

static int print_vector(const char* tag, graphblas::Vector<float>* v, int n) {
  std::vector<float> h(n, -1.f);
  graphblas::Index size = n;
  if (v->extractTuples(&h, &size) != graphblas::GrB_SUCCESS) return 1;
  printf("%s", tag);
  for (int i = 0; i < n; ++i) {
    unsigned int bits;
    memcpy(&bits, &h[i], 4);
    printf(" %08x", bits);
  }
  printf("\n");
  return 0;
}

static void print_record(const char* tag, const grb_lcc_result& rec) {
  printf("%s %lld %lld %lld %lld %d\n", tag, static_cast<long long>(rec.edges), static_cast<long long>(rec.triangles),
         static_cast<long long>(rec.closed), static_cast<long long>(rec.wedges), rec.max_degree);
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
  Vector<float> lcc(7);
  Descriptor desc;
  grb_lcc_result rec;
  if (algorithm::lcc(&lcc, &a, false, &desc, &rec) != GrB_SUCCESS) return 4;
  if (print_vector("und", &lcc, 7)) return 4;
  print_record("rec", rec);

  std::vector<Index> dr, dc;
  std::vector<int> dv;
  const int d[][2] = {{0, 1}, {1, 0}, {1, 2}, {2, 0}, {0, 3}, {3, 1}, {3, 3}};
  for (size_t i = 0; i < sizeof(d) / sizeof(d[0]); ++i) { dr.push_back(d[i][0]); dc.push_back(d[i][1]); dv.push_back(static_cast<int>(i) - 1); }
  Matrix<int> b(5, 5);
  if (b.build(&dr, &dc, &dv, static_cast<Index>(dr.size()), GrB_NULL) != GrB_SUCCESS) return 3;
  const Matrix<int>* cb = &b;
  Vector<float> l5(5);
  grb_lcc_result drec;
  if (algorithm::lcc(&l5, cb, true, static_cast<Descriptor*>(NULL), &drec) != GrB_SUCCESS) return 5;
  if (print_vector("dir", &l5, 5)) return 5;
  print_record("drec", drec);
  printf("asym %d\n", algorithm::lcc(&l5, cb, false, &desc) == GrB_INVALID_VALUE ? 1 : 0);
  return 0;
}
