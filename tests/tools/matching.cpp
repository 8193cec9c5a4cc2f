// Test driver: algorithm::matching through the drop-in frontend.  Reads an .mtx file with readMtx, keeps its off-diagonal
// entries in both directions, gives the edge {u, v} the weight 1 + (min + 3 max) % 7, and runs the matching on a float matrix
// heaviest first (a descriptor, C, the record), on a const int matrix lightest first (a NULL descriptor, a NULL C, no record)
// and hashed with seed 5, then heaviest first in place.  Prints, a line each,
//   "heaviest edges E matched M weight W exposed X isolated I launches L"
//   "mate ..."                                  the partners after the float run
//   "csr | pointers | indices | values"         C's CSR after the float run
//   "lightest mate ..." and "hashed mate ..."   after the int runs
// and "ok" when the in-place run agrees with the float run; tests/test_gpu_matching.py compares the lines with its greedy scan.
#define GRB_USE_CUDA
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/matching.hpp"

static bool print_mate(const char* name, graphblas::Vector<int>* mate, graphblas::Index n) {
  std::vector<int> h(n, -7);
  graphblas::Index size = n;
  if (mate->extractTuples(&h, &size) != graphblas::GrB_SUCCESS || size != n) return false;
  printf("%s", name);
  for (graphblas::Index i = 0; i < n; ++i) printf(" %d", h[i]);
  printf("\n");
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using namespace graphblas;
  std::vector<Index> r, c;
  std::vector<float> v;
  Index nr, nc, nv;
  readMtx(argv[1], &r, &c, &v, &nr, &nc, &nv, 1, false, NULL);
  if (nr != nc) return 2;
  std::set<std::pair<Index, Index> > both;
  for (Index i = 0; i < nv; ++i)
    if (r[i] != c[i]) {
      both.insert(std::make_pair(r[i], c[i]));
      both.insert(std::make_pair(c[i], r[i]));
    }
  std::vector<Index> sr, sc;
  std::vector<float> sf;
  std::vector<int> si;
  for (std::set<std::pair<Index, Index> >::const_iterator it = both.begin(); it != both.end(); ++it) {
    const Index lo = std::min(it->first, it->second), hi = std::max(it->first, it->second);
    sr.push_back(it->first);
    sc.push_back(it->second);
    si.push_back(1 + (lo + 3 * hi) % 7);
    sf.push_back(static_cast<float>(si.back()));
  }
  const Index ne = static_cast<Index>(sr.size());

  Matrix<float> a(nr, nr), m(nr, nr);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> mate(nr);
  Descriptor desc;
  grb_matching_result rec;
  if (algorithm::matching(&mate, &m, &a, GRB_MATCH_HEAVIEST, 0u, &desc, &rec) != GrB_SUCCESS) return 4;
  printf("heaviest edges %lld matched %lld weight %.17g exposed %d isolated %d launches %d\n", static_cast<long long>(rec.edges),
         static_cast<long long>(rec.matched), rec.weight, rec.exposed, rec.isolated, rec.launches);
  if (!print_mate("mate", &mate, nr)) return 5;
  const grb_index *ptr, *ind;
  const void* val;
  grb_index mnv = 0;
  grb_matrix_nvals(m.handle(), &mnv);
  if (grb_matrix_host_csr(m.handle(), &ptr, &ind, &val) != 0) return 6;
  printf("csr |");
  for (Index i = 0; i <= nr; ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < mnv; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (grb_index i = 0; i < mnv; ++i) printf(" %g", static_cast<const float*>(val)[i]);
  printf("\n");

  Matrix<int> b(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 7;
  const Matrix<int>* cb = &b;
  Vector<int> mate2(nr);
  if (algorithm::matching(&mate2, static_cast<Matrix<int>*>(NULL), cb, GRB_MATCH_LIGHTEST, 0u, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS)
    return 8;
  if (!print_mate("lightest mate", &mate2, nr)) return 9;
  if (algorithm::matching(&mate2, static_cast<Matrix<int>*>(NULL), cb, GRB_MATCH_HASHED, 5u, &desc) != GrB_SUCCESS) return 10;
  if (!print_mate("hashed mate", &mate2, nr)) return 11;
  grb_matching_result irec;
  if (algorithm::matching(&mate2, &b, cb, GRB_MATCH_HEAVIEST, 0u, &desc, &irec) != GrB_SUCCESS) return 12;   // in place: b becomes its matching
  grb_index bnv = 0;
  grb_matrix_nvals(b.handle(), &bnv);
  if (bnv != mnv || irec.matched != rec.matched || irec.weight != rec.weight || irec.exposed != rec.exposed) return 13;
  Matrix<float> wrong(nr, nr);                                                    // C not of A's type
  if (to_info(grb_matching(mate2.handle(), wrong.handle(), b.handle(), 0, 0u, NULL, NULL)) != GrB_DOMAIN_MISMATCH) return 14;
  if (to_info(grb_matching(mate2.handle(), NULL, b.handle(), 3, 0u, NULL, NULL)) != GrB_INVALID_VALUE) return 15;
  printf("ok\n");
  return 0;
}
