// Test driver: algorithm::random_walk and algorithm::sample_neighbors through the drop-in frontend.  Reads an .mtx file with
// readMtx, keeps its off-diagonal entries in both directions, and works on a float matrix whose values are 1 + (i + j) % 3
// and on a const int matrix with the same integers.  Prints, a line each,
//   "uniform walkers W steps S dead D |" and the walks      every vertex a walker (a NULL list), length 6, seed 11, a descriptor
//   "weighted walkers W steps S dead D |" and the walks     the starts n - 1, 0, 0, 3, length 9, seed 12, a NULL descriptor
//   "sample rows R entries E full F | ptr | ind | val"      the seeds n - 1, 0, 0, 5, 2, fanout 3, seed 13
// and "ok" when the int runs agree with the float runs and the error paths leave their outputs alone;
// tests/test_gpu_sample.py compares the lines with its model.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/random_walk.hpp"
#include "graphblas/algorithm/sample_neighbors.hpp"

static int values_of(const char* name, const grb_walk_result* rec, graphblas::Vector<int>* v, graphblas::Index size, std::vector<int>* h) {
  h->assign(size, -7);
  graphblas::Index n = size;
  if (v->extractTuples(h, &n) != graphblas::GrB_SUCCESS || n != size) return 1;
  if (name) {
    printf("%s walkers %lld steps %lld dead %lld |", name, static_cast<long long>(rec->walkers), static_cast<long long>(rec->steps),
           static_cast<long long>(rec->dead_ends));
    for (graphblas::Index i = 0; i < size; ++i) printf(" %d", (*h)[i]);
    printf("\n");
  }
  return 0;
}

template <typename T>
static int csr_of(graphblas::Matrix<T>* c, graphblas::Index rows, std::vector<int>* ptr, std::vector<int>* ind, std::vector<double>* val) {
  const grb_index *p, *i;
  const void* v;
  grb_index nv = 0;
  grb_matrix_nvals(c->handle(), &nv);
  if (grb_matrix_host_csr(c->handle(), &p, &i, &v) != 0) return 1;
  ptr->assign(p, p + rows + 1);
  ind->assign(i, i + nv);
  val->clear();
  for (grb_index k = 0; k < nv; ++k) val->push_back(static_cast<double>(static_cast<const T*>(v)[k]));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using namespace graphblas;
  std::vector<Index> r, c;
  std::vector<float> v;
  Index nr, nc, nv;
  readMtx(argv[1], &r, &c, &v, &nr, &nc, &nv, 1, false, NULL);
  if (nr != nc || nr < 6) return 2;
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
  Matrix<int> b(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  const Matrix<int>* cb = &b;
  Descriptor desc;

  // ---- the walks
  const int ulen = 6, wlen = 9;
  Vector<int> uw(nr * (ulen + 1)), uwi(nr * (ulen + 1));
  grb_walk_result urec, wrec;
  if (algorithm::random_walk(&uw, &a, static_cast<const std::vector<Index>*>(NULL), ulen, GRB_WALK_UNIFORM, 11u, &desc, &urec) != GrB_SUCCESS)
    return 4;
  std::vector<int> hu, hw, hi;
  if (values_of("uniform", &urec, &uw, nr * (ulen + 1), &hu)) return 5;
  if (algorithm::random_walk(&uwi, cb, static_cast<const std::vector<Index>*>(NULL), ulen, GRB_WALK_UNIFORM, 11u, &desc) != GrB_SUCCESS) return 4;
  if (values_of(NULL, NULL, &uwi, nr * (ulen + 1), &hi) || hi != hu) return 6;
  std::vector<Index> starts;
  starts.push_back(nr - 1);
  starts.push_back(0);
  starts.push_back(0);
  starts.push_back(3);
  const Index wsize = static_cast<Index>(starts.size()) * (wlen + 1);
  Vector<int> ww(wsize), wwi(wsize);
  if (algorithm::random_walk(&ww, &a, &starts, wlen, GRB_WALK_WEIGHTED, 12u, static_cast<Descriptor*>(NULL), &wrec) != GrB_SUCCESS) return 7;
  if (values_of("weighted", &wrec, &ww, wsize, &hw)) return 5;
  if (algorithm::random_walk(&wwi, cb, &starts, wlen, GRB_WALK_WEIGHTED, 12u, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 7;
  if (values_of(NULL, NULL, &wwi, wsize, &hi) || hi != hw) return 6;
  // errors leave walks alone
  if (algorithm::random_walk(&ww, &a, &starts, wlen, 2, 12u, &desc) != GrB_INVALID_VALUE) return 8;
  if (algorithm::random_walk(&ww, &a, &starts, wlen + 1, GRB_WALK_UNIFORM, 12u, &desc) != GrB_DIMENSION_MISMATCH) return 8;
  starts[2] = nr;
  if (algorithm::random_walk(&ww, &a, &starts, wlen, GRB_WALK_UNIFORM, 12u, &desc) != GrB_INVALID_INDEX) return 8;
  if (values_of(NULL, NULL, &ww, wsize, &hi) || hi != hw) return 9;

  // ---- the sample
  std::vector<Index> seeds;
  seeds.push_back(nr - 1);
  seeds.push_back(0);
  seeds.push_back(0);
  seeds.push_back(5);
  seeds.push_back(2);
  const Index ns = static_cast<Index>(seeds.size());
  Matrix<float> cf(ns, nr);
  Matrix<int> ci(ns, nr);
  grb_sample_result srec;
  if (algorithm::sample_neighbors(&cf, &a, &seeds, 3, 13u, &desc, &srec) != GrB_SUCCESS) return 10;
  if (algorithm::sample_neighbors(&ci, cb, &seeds, 3, 13u, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 10;
  std::vector<int> fp, fi, ip, ii;
  std::vector<double> fv, iv;
  if (csr_of(&cf, ns, &fp, &fi, &fv) || csr_of(&ci, ns, &ip, &ii, &iv)) return 11;
  if (fp != ip || fi != ii || fv != iv) return 12;
  printf("sample rows %lld entries %lld full %lld |", static_cast<long long>(srec.rows), static_cast<long long>(srec.entries),
         static_cast<long long>(srec.full_rows));
  for (size_t k = 0; k < fp.size(); ++k) printf(" %d", fp[k]);
  printf(" |");
  for (size_t k = 0; k < fi.size(); ++k) printf(" %d", fi[k]);
  printf(" |");
  for (size_t k = 0; k < fv.size(); ++k) printf(" %g", fv[k]);
  printf("\n");
  // errors leave C alone
  if (algorithm::sample_neighbors(&cf, &a, &seeds, 0, 13u, &desc) != GrB_INVALID_VALUE) return 13;
  seeds[1] = nr;
  if (algorithm::sample_neighbors(&cf, &a, &seeds, 3, 13u, &desc) != GrB_INDEX_OUT_OF_BOUNDS) return 13;
  if (csr_of(&cf, ns, &ip, &ii, &iv) || fp != ip || fi != ii || fv != iv) return 14;
  printf("ok\n");
  return 0;
}
