// Test driver: algorithm::relabel and algorithm::contract through the drop-in frontend.  Reads an .mtx file with readMtx, keeps
// its entries in both directions (the diagonal too), gives the entry (r, c) the value 1 + (r + 3 c) % 7, and contracts
//   a float matrix by the pairs map(v) = v / 2 under GRB_OP_PLUS without loops (a descriptor, sizes, the record),
//   a const int matrix by map(v) = v % 5, or -1 where v % 11 == 0, under GRB_OP_MAXIMUM with loops (a NULL descriptor),
// and relabels the labels 3 (v / 4).  Prints, a line each,
//   "pairs kept K loops L entries E clusters C dropped D largest G | pointers | indices | values | sizes"
//   "communities ..."                           the same for the int run
//   "relabel COUNT | map ..."
// and "ok" when the error codes asked for at the end come back; tests/test_gpu_contract.py compares the lines with numpy.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/contract.hpp"

template <typename T>
static bool print_run(const char* name, graphblas::Matrix<T>* c, graphblas::Vector<int>* sizes, graphblas::Index nc,
                      const grb_contract_result& rec) {
  const grb_index *ptr, *ind;
  const void* val;
  grb_index nv = 0;
  grb_matrix_nvals(c->handle(), &nv);
  if (grb_matrix_host_csr(c->handle(), &ptr, &ind, &val) != 0) return false;
  printf("%s kept %lld loops %lld entries %lld clusters %d dropped %d largest %d |", name, static_cast<long long>(rec.kept),
         static_cast<long long>(rec.loops), static_cast<long long>(rec.entries), rec.clusters, rec.dropped, rec.largest);
  for (graphblas::Index i = 0; i <= nc; ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %g", static_cast<double>(static_cast<const T*>(val)[i]));
  printf(" |");
  std::vector<int> h(nc, -7);
  graphblas::Index size = nc;
  if (sizes->extractTuples(&h, &size) != graphblas::GrB_SUCCESS || size != nc) return false;
  for (graphblas::Index i = 0; i < nc; ++i) printf(" %d", h[i]);
  printf("\n");
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using namespace graphblas;
  std::vector<Index> r, c;
  std::vector<float> v;
  Index nr, ncol, nv;
  readMtx(argv[1], &r, &c, &v, &nr, &ncol, &nv, 1, false, NULL);
  if (nr != ncol) return 2;
  std::set<std::pair<Index, Index> > both;
  for (Index i = 0; i < nv; ++i) {
    both.insert(std::make_pair(r[i], c[i]));
    both.insert(std::make_pair(c[i], r[i]));
  }
  std::vector<Index> sr, sc;
  std::vector<float> sf;
  std::vector<int> si;
  for (std::set<std::pair<Index, Index> >::const_iterator it = both.begin(); it != both.end(); ++it) {
    sr.push_back(it->first);
    sc.push_back(it->second);
    si.push_back(1 + (it->first + 3 * it->second) % 7);
    sf.push_back(static_cast<float>(si.back()));
  }
  const Index ne = static_cast<Index>(sr.size());
  const Index n = nr;

  // pairs: PLUS without loops on a float matrix
  const Index np = (n + 1) / 2;
  std::vector<int> pairs(n), comm(n), labels(n);
  for (Index i = 0; i < n; ++i) {
    pairs[i] = i / 2;
    comm[i] = i % 11 == 0 ? -1 : i % 5;
    labels[i] = 3 * (i / 4);
  }
  Matrix<float> a(n, n), cp(np, np);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> map(n), sizes(np);
  if (map.build(&pairs, n) != GrB_SUCCESS) return 3;
  Descriptor desc;
  grb_contract_result rec;
  if (algorithm::contract(&cp, &sizes, &a, &map, GRB_OP_PLUS, 0, &desc, &rec) != GrB_SUCCESS) return 4;
  if (!print_run("pairs", &cp, &sizes, np, rec)) return 5;

  // communities: MAXIMUM with loops on a const int matrix, a NULL descriptor
  Matrix<int> b(n, n), cc(5, 5);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 6;
  const Matrix<int>* cb = &b;
  Vector<int> map2(n), sizes2(5);
  if (map2.build(&comm, n) != GrB_SUCCESS) return 6;
  const Vector<int>* cmap2 = &map2;
  grb_contract_result rec2;
  if (algorithm::contract(&cc, &sizes2, cb, cmap2, GRB_OP_MAXIMUM, 1, static_cast<Descriptor*>(NULL), &rec2) != GrB_SUCCESS) return 7;
  if (!print_run("communities", &cc, &sizes2, 5, rec2)) return 8;
  // ... and without sizes and record: the same entries
  Matrix<int> cc2(5, 5);
  if (algorithm::contract(&cc2, static_cast<Vector<int>*>(NULL), cb, cmap2, GRB_OP_MAXIMUM, 1, &desc) != GrB_SUCCESS) return 9;
  grb_index n1 = 0, n2 = 0;
  grb_matrix_nvals(cc.handle(), &n1);
  grb_matrix_nvals(cc2.handle(), &n2);
  if (n1 != n2 || static_cast<long long>(n1) != static_cast<long long>(rec2.entries)) return 10;

  // relabel
  Vector<int> lab(n), dense(n);
  if (lab.build(&labels, n) != GrB_SUCCESS) return 11;
  int count = -1;
  if (algorithm::relabel(&dense, &lab, GRB_RELABEL_LABELS, &count) != GrB_SUCCESS) return 12;
  std::vector<int> h(n, -7);
  Index size = n;
  if (dense.extractTuples(&h, &size) != GrB_SUCCESS || size != n) return 13;
  printf("relabel %d |", count);
  for (Index i = 0; i < n; ++i) printf(" %d", h[i]);
  printf("\n");
  if (algorithm::relabel(&lab, &lab, GRB_RELABEL_MATE) != GrB_SUCCESS) return 14;                // in place, no count

  // errors
  Matrix<float> wrong(5, 5);                                                                      // a float C is fine with the float A ...
  if (algorithm::contract(&wrong, static_cast<Vector<int>*>(NULL), &a, cmap2, GRB_OP_FIRST, 0, &desc) != GrB_SUCCESS) return 15;
  // ... and not with the int A
  if (to_info(grb_contract(wrong.handle(), NULL, b.handle(), map2.handle(), GRB_OP_PLUS, 0, NULL, NULL)) != GrB_DOMAIN_MISMATCH) return 16;
  if (to_info(grb_contract(cc.handle(), NULL, b.handle(), map2.handle(), GRB_OP_MULTIPLIES, 0, NULL, NULL)) != GrB_NOT_IMPLEMENTED) return 17;
  if (to_info(grb_contract(cc.handle(), NULL, b.handle(), map2.handle(), GRB_OP_PLUS, 2, NULL, NULL)) != GrB_INVALID_VALUE) return 18;
  if (to_info(grb_contract(cc.handle(), NULL, b.handle(), map.handle(), GRB_OP_PLUS, 0, NULL, NULL)) != GrB_INVALID_INDEX) return 19;   // pairs: ids past 4
  if (to_info(grb_relabel(dense.handle(), lab.handle(), 2, NULL, NULL)) != GrB_INVALID_VALUE) return 20;
  printf("ok\n");
  return 0;
}
