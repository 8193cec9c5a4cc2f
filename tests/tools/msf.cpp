// Test driver: algorithm::msf through the drop-in frontend.  Reads an .mtx file with readMtx, keeps its off-diagonal entries
// in both directions with unit weights, and runs the minimum spanning forest on a float matrix (a descriptor, comp, the
// record) and on a const int matrix (a NULL descriptor, a NULL comp, no record; then in place).  Prints, a line each,
//   "float edges E forest F weight W components K isolated I launches L"
//   "csr | pointers | indices"                  C's CSR after the float run
//   "comp ..."                                  the component labels
//   "int forest F nvals NV"                     after the int run
// and "ok" when the int runs agree with the float run; tests/test_gpu_msf.py compares the lines with its Kruskal.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/msf.hpp"

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
    sr.push_back(it->first);
    sc.push_back(it->second);
    sf.push_back(1.f);
    si.push_back(1);
  }
  const Index ne = static_cast<Index>(sr.size());

  Matrix<float> a(nr, nr), forest(nr, nr);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> comp(nr);
  Descriptor desc;
  grb_msf_result rec;
  if (algorithm::msf(&forest, &comp, &a, &desc, &rec) != GrB_SUCCESS) return 4;
  printf("float edges %lld forest %lld weight %.17g components %d isolated %d launches %d\n", static_cast<long long>(rec.edges),
         static_cast<long long>(rec.forest_edges), rec.weight, rec.components, rec.isolated, rec.launches);
  const grb_index *ptr, *ind;
  const void* val;
  grb_index fnv = 0;
  grb_matrix_nvals(forest.handle(), &fnv);
  if (grb_matrix_host_csr(forest.handle(), &ptr, &ind, &val) != 0) return 5;
  printf("csr |");
  for (Index i = 0; i <= nr; ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < fnv; ++i) printf(" %d", ind[i]);
  printf("\n");
  for (grb_index i = 0; i < fnv; ++i)
    if (static_cast<const float*>(val)[i] != 1.f) return 6;
  std::vector<int> h(nr, -1);
  Index size = nr;
  if (comp.extractTuples(&h, &size) != GrB_SUCCESS || size != nr) return 7;
  printf("comp");
  for (Index i = 0; i < nr; ++i) printf(" %d", h[i]);
  printf("\n");

  Matrix<int> b(nr, nr), iforest(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 8;
  const Matrix<int>* cb = &b;
  if (algorithm::msf(&iforest, static_cast<Vector<int>*>(NULL), cb, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 9;
  grb_index inv = 0;
  grb_matrix_nvals(iforest.handle(), &inv);
  grb_msf_result irec;
  if (algorithm::msf(&b, &comp, cb, &desc, &irec) != GrB_SUCCESS) return 10;      // in place: b becomes its forest
  grb_index bnv = 0;
  grb_matrix_nvals(b.handle(), &bnv);
  printf("int forest %lld nvals %d\n", static_cast<long long>(irec.forest_edges), inv);
  if (inv != fnv || bnv != fnv || irec.forest_edges != rec.forest_edges || irec.weight != rec.weight || irec.components != rec.components)
    return 11;
  Matrix<float> wrong(nr, nr);                                                    // C not of A's type
  if (to_info(grb_msf(wrong.handle(), NULL, b.handle(), NULL, NULL)) != GrB_DOMAIN_MISMATCH) return 12;
  printf("ok\n");
  return 0;
}
