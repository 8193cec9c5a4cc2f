// Test driver: algorithm::louvain through the drop-in frontend.  Reads an .mtx file with readMtx, keeps its off-diagonal
// entries in both directions, and runs Louvain on a float matrix whose values are 1 + (i + j) % 3 (a descriptor, the record,
// weighted = 1 and weighted = 0) and on a const int matrix with the same integers (a NULL descriptor, no record).  Prints, a
// line each,
//   "weighted levels L rounds R moves M proposals P communities K qn Q w W launches N"
//   "labels ..."                                the weighted run's labels
//   "unweighted levels L rounds R moves M proposals P communities K qn Q w W launches N"
//   "ulabels ..."                               the unweighted run's labels
// and "ok" when the int run agrees with the float run; tests/test_gpu_louvain.py compares the lines with its model.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/louvain.hpp"

static void line(const char* name, const grb_louvain_result& r) {
  printf("%s levels %d rounds %d moves %lld proposals %lld communities %d qn %lld w %lld launches %d\n", name, r.levels, r.rounds,
         static_cast<long long>(r.moves), static_cast<long long>(r.proposals), r.communities, static_cast<long long>(r.qn),
         static_cast<long long>(r.w), r.launches);
}

static int labels_of(const char* name, graphblas::Vector<int>* v, graphblas::Index nr, std::vector<int>* h) {
  h->assign(nr, -1);
  graphblas::Index size = nr;
  if (v->extractTuples(h, &size) != graphblas::GrB_SUCCESS || size != nr) return 1;
  if (name) {
    printf("%s", name);
    for (graphblas::Index i = 0; i < nr; ++i) printf(" %d", (*h)[i]);
    printf("\n");
  }
  return 0;
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
    sr.push_back(it->first);
    sc.push_back(it->second);
    si.push_back(1 + (it->first + it->second) % 3);
    sf.push_back(static_cast<float>(si.back()));
  }
  const Index ne = static_cast<Index>(sr.size());

  Matrix<float> a(nr, nr);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> lab(nr), ulab(nr), ilab(nr);
  Descriptor desc;
  grb_louvain_result rec, urec;
  if (algorithm::louvain(&lab, &a, 1, 100, 1000000, &desc, &rec) != GrB_SUCCESS) return 4;
  if (algorithm::louvain(&ulab, &a, 0, 100, 1000000, &desc, &urec) != GrB_SUCCESS) return 4;
  std::vector<int> h, hu, hi;
  line("weighted", rec);
  if (labels_of("labels", &lab, nr, &h)) return 5;
  line("unweighted", urec);
  if (labels_of("ulabels", &ulab, nr, &hu)) return 5;
  if (rec.modularity != static_cast<double>(rec.qn) / (static_cast<double>(rec.w) * static_cast<double>(rec.w))) return 6;

  Matrix<int> b(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 7;
  const Matrix<int>* cb = &b;
  if (algorithm::louvain(&ilab, cb, 1, 100, 1000000, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 8;
  if (labels_of(NULL, &ilab, nr, &hi) || hi != h) return 9;
  if (to_info(grb_louvain(lab.handle(), a.handle(), 2, 1, 1, NULL, NULL)) != GrB_INVALID_VALUE) return 10;
  if (to_info(grb_louvain(lab.handle(), a.handle(), 1, 0, 1, NULL, NULL)) != GrB_INVALID_VALUE) return 10;
  if (labels_of(NULL, &lab, nr, &hi) || hi != h) return 11;                         // labels keeps what it held
  printf("ok\n");
  return 0;
}
