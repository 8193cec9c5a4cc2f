// Test driver: algorithm::maxflow through the drop-in frontend.  Reads an .mtx file with readMtx, keeps its off-diagonal
// entries in both directions, gives the arc i -> j the capacity 1 + (i + 3 j) % 7, and runs the maximum flow from vertex 0 to
// vertex n - 1 on a float matrix (a descriptor, F, side, the record), on a const int matrix (a NULL descriptor, a NULL F, no
// record), with unit capacities (a NULL side), then on the int matrix in place.  Prints, a line each,
//   "capacity value V arcs A flow_arcs M sink_side S cut_arcs K cut_capacity C launches L"
//   "side ..."                                  after the float run
//   "csr | pointers | indices | values"         F's CSR after the float run
//   "int side ..."                              after the int run
//   "unit value V flow_arcs M"
// and "ok" when the in-place run agrees with the float run; tests/test_gpu_maxflow.py compares the lines with scipy's value
// and its own residual reachability, and checks that F is a maximum flow.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/maxflow.hpp"

static bool print_side(const char* name, graphblas::Vector<int>* side, graphblas::Index n) {
  std::vector<int> h(n, -7);
  graphblas::Index size = n;
  if (side->extractTuples(&h, &size) != graphblas::GrB_SUCCESS || size != n) return false;
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
  if (nr != nc || nr < 2) return 2;
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
    si.push_back(1 + (it->first + 3 * it->second) % 7);
    sf.push_back(static_cast<float>(si.back()));
  }
  const Index ne = static_cast<Index>(sr.size());
  const Index source = 0, sink = nr - 1;

  Matrix<float> a(nr, nr), f(nr, nr);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> side(nr);
  Descriptor desc;
  grb_maxflow_result rec;
  if (algorithm::maxflow(&f, &side, &a, source, sink, GRB_FLOW_CAPACITY, &desc, &rec) != GrB_SUCCESS) return 4;
  printf("capacity value %lld arcs %lld flow_arcs %lld sink_side %lld cut_arcs %lld cut_capacity %lld launches %d\n",
         static_cast<long long>(rec.value), static_cast<long long>(rec.arcs), static_cast<long long>(rec.flow_arcs),
         static_cast<long long>(rec.sink_side), static_cast<long long>(rec.cut_arcs), static_cast<long long>(rec.cut_capacity), rec.launches);
  if (!print_side("side", &side, nr)) return 5;
  const grb_index *ptr, *ind;
  const void* val;
  grb_index fnv = 0;
  grb_matrix_nvals(f.handle(), &fnv);
  if (grb_matrix_host_csr(f.handle(), &ptr, &ind, &val) != 0) return 6;
  printf("csr |");
  for (Index i = 0; i <= nr; ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < fnv; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (grb_index i = 0; i < fnv; ++i) printf(" %g", static_cast<const float*>(val)[i]);
  printf("\n");

  Matrix<int> b(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 7;
  const Matrix<int>* cb = &b;
  Vector<int> side2(nr);
  if (algorithm::maxflow(static_cast<Matrix<int>*>(NULL), &side2, cb, source, sink, GRB_FLOW_CAPACITY, static_cast<Descriptor*>(NULL)) !=
      GrB_SUCCESS)
    return 8;
  if (!print_side("int side", &side2, nr)) return 9;
  grb_maxflow_result urec;
  Matrix<int> uf(nr, nr);
  if (algorithm::maxflow(&uf, static_cast<Vector<int>*>(NULL), cb, source, sink, GRB_FLOW_UNIT, &desc, &urec) != GrB_SUCCESS) return 10;
  printf("unit value %lld flow_arcs %lld\n", static_cast<long long>(urec.value), static_cast<long long>(urec.flow_arcs));
  grb_maxflow_result irec;
  if (algorithm::maxflow(&b, &side2, cb, source, sink, GRB_FLOW_CAPACITY, &desc, &irec) != GrB_SUCCESS) return 11;   // in place: b becomes its flow
  grb_index bnv = 0;
  grb_matrix_nvals(b.handle(), &bnv);
  if (bnv != fnv || irec.value != rec.value || irec.flow_arcs != rec.flow_arcs || irec.cut_arcs != rec.cut_arcs ||
      irec.cut_capacity != rec.value || irec.sink_side != rec.sink_side)
    return 12;
  Matrix<float> wrong(nr, nr);                                                    // F not of A's type
  Matrix<int> b2(nr, nr);
  if (b2.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 13;
  if (to_info(grb_maxflow(wrong.handle(), NULL, b2.handle(), 0, 1, 0, NULL, NULL)) != GrB_DOMAIN_MISMATCH) return 14;
  if (to_info(grb_maxflow(NULL, NULL, b2.handle(), 0, 1, 2, NULL, NULL)) != GrB_INVALID_VALUE) return 15;
  if (to_info(grb_maxflow(NULL, NULL, b2.handle(), 0, 0, 0, NULL, NULL)) != GrB_INVALID_VALUE) return 16;
  if (to_info(grb_maxflow(NULL, NULL, b2.handle(), 0, nr, 0, NULL, NULL)) != GrB_INDEX_OUT_OF_BOUNDS) return 17;
  printf("ok\n");
  return 0;
}
